"""Register budget of the tiled missing-value fill (dctz_kernels_ndmask.hip): exactly the intended instantiations of
k_ndmask_fill are built -- T in {double, float} x geometry in {2-D, 3-D} -- and each runs without scratch, without spilled
VGPRs and without LDS, in few enough registers for eight waves per SIMD like the flat kernel (read from the code object's
metadata).  Built: 56 VGPRs (fp64 2-D: 57), no AGPRs, LDS 0."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")
GEOM_2D, GEOM_3D = 1, 2                       # dct_nd_block.h


@pytest.fixture(scope="module", autouse=True)
def built():
    """A missing library is built, as tests/test_abi_cpu.py does; one that does not build fails the test."""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def test_ndmask_kernels_have_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::k_ndmask")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::k_ndmask_fill<{t}, {g}>" for t in ("double", "float") for g in (GEOM_2D, GEOM_3D)]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k.get("group_segment_fixed_size", 0) == 0, k
        # eight waves per SIMD: 512 registers per lane of a SIMD, VGPRs and AGPRs together
        assert k["vgpr_count"] + k.get("agpr", 0) <= 64, k
