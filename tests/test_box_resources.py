"""Register budget of the box decode (dctz_kernels_box.hip): every k_decompress_box* instantiation is built, and runs
without scratch and without spilled VGPRs (read from the code object's metadata)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_box_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::k_decompress_box")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::k_decompress_box{r}<{t}, {m}>" for r in ("", "_rem") for t in ("double", "float") for m in (0, 1)]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
