"""Register budget of the rate-distortion probe (dctz_kernels_rd.hip): a lane holds a whole block, so every built
k_rd_probe instantiation must run without scratch and without spilled VGPRs (read from the code object's metadata)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_rd_probe_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if "k_rd_probe" in k.get("demangled", "")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    assert any("k_rd_probe<double>" in n for n in names) and any("k_rd_probe<float>" in n for n in names), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
