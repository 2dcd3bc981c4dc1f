"""Register budget of the list decoders of coarse boxes (dctz_kernels_mcboxnd.hip): exactly the intended instantiations are
built -- dctz::tiled::k_ndcoarse_mbox for T x MODE x (8 x 8: K = 2, 4; 4 x 4 x 4: K = 2), the DC-only gather per T -- and each
runs without scratch and without spilled VGPRs (read from the code object's metadata).  The single call's kernels
(dctz::k_ndcoarse_box...) and the full-resolution list decoder (dctz::tiled::k_decompress_mbox_nd) keep prefixes of their own."""
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


def test_ndcoarse_mbox_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::tiled::k_ndcoarse_mbox")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    types, modes = ("double", "float"), (0, 1)
    want = [f"dctz::tiled::k_ndcoarse_mbox<{t}, {m}, {g}, {k}>" for t in types for m in modes for g, k in ((1, 2), (1, 4), (2, 2))]
    want += [f"dctz::tiled::k_ndcoarse_mbox_dc<{t}>" for t in types]
    assert len(want) == 14
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
