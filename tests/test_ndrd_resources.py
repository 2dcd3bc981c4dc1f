"""Register budget of the tiled rate-distortion probe (dctz_kernels_ndrd.hip): a lane of k_ndrd_probe holds a whole tile, so all
four instantiations (fp64 / fp32 x 8 x 8 / 4 x 4 x 4) must be built and run without scratch and without spilled VGPRs (read from
the code object's metadata).  k_ndrd_edge, the pass over the tiles with padding, is reported only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


def test_ndrd_probe_kernels_have_no_scratch():
    assert os.path.exists(LIB), "libdctzhip.so is not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if "k_ndrd_" in k.get("demangled", "")]
    probe = [k for k in ks if "k_ndrd_probe<" in k["demangled"]]
    names = sorted(k["demangled"].split("(")[0] for k in probe)
    for want in ("k_ndrd_probe<double, 1>", "k_ndrd_probe<double, 2>", "k_ndrd_probe<float, 1>", "k_ndrd_probe<float, 2>"):
        assert sum(want in n for n in names) == 1, (want, names)
    assert len(probe) == 4, names
    for k in probe:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
    for k in ks:
        print(k["demangled"].split("(")[0], {f: k.get(f) for f in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                                                     "vgpr_spill_count", "sgpr_spill_count")})
