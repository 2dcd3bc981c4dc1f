"""Register budget of random access on decode (dctz_kernels_ra.hip): every k_ac_index* and k_decompress_range*
instantiation is built, and runs without scratch and without spilled VGPRs (read from the code object's metadata)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_range_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith(("dctz::k_ac_index", "dctz::k_decompress_range"))]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = ["dctz::k_ac_index", "dctz::k_ac_index_scan", "dctz::k_ac_index_add"]
    for t in ("double", "float"):
        for m in (0, 1):
            want += [f"dctz::k_decompress_range<{t}, {m}>", f"dctz::k_decompress_range_rem<{t}, {m}>"]
    for w in want:
        assert w in names, (w, names)
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
