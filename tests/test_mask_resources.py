"""Register budget of the missing-value layer (dctz_kernels_mask.hip): exactly the intended instantiations are built -- T of
k_mask_fill and of k_mask_apply, no short-block form (the fill kernel covers the short block itself) -- and each runs without
scratch, without spilled VGPRs and without LDS, in few enough registers for eight waves per SIMD (read from the code
object's metadata)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.fixture(scope="module", autouse=True)
def built():
    """A missing library is built, as tests/test_abi_cpu.py does; one that does not build fails the test."""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def test_mask_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::k_mask")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::{k}<{t}>" for k in ("k_mask_fill", "k_mask_apply") for t in ("double", "float")]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k.get("group_segment_fixed_size", 0) == 0, k
        # eight waves per SIMD: 512 registers per lane of a SIMD, VGPRs and AGPRs together
        assert k["vgpr_count"] + k.get("agpr", 0) <= 64, k
