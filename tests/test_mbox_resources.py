"""Register budget of the list-of-boxes decode (dctz_kernels_mbox.hip): the list builder and every k_decompress_mbox*
instantiation are built, and run without scratch and without spilled VGPRs (read from the code object's metadata)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_mbox_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    all_ks = kernels_of(LIB)
    ks = [k for k in all_ks if k.get("demangled", "").startswith("dctz::k_decompress_mbox")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::k_decompress_mbox{r}<{t}, {m}>" for r in ("", "_rem") for t in ("double", "float") for m in (0, 1)]
    assert names == sorted(want), names
    build = [k for k in all_ks if k.get("demangled", "").split("(")[0] == "dctz::k_boxlist_build"]
    assert len(build) == 1, [k.get("demangled") for k in all_ks if "boxlist" in k.get("demangled", "")]
    for k in ks + build:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
