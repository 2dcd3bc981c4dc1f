"""Register budget of the correction list (dctz_kernels_fixup.hip): exactly the intended instantiations are built -- T x MODE of
k_fixup_mark and of k_fixup_mark_rem, T of k_fixup_emit and of k_fixup_apply, and k_fixup_scan -- and each runs without
scratch and without spilled VGPRs (read from the code object's metadata).  The mark kernels keep the LDS of the summaries'
form with an original: 16 KiB at the most."""
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


def test_fixup_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::k_fixup")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    types, modes = ("double", "float"), (0, 1)
    want = [f"dctz::{k}<{t}, {m}>" for k in ("k_fixup_mark", "k_fixup_mark_rem") for t in types for m in modes]
    want += [f"dctz::{k}<{t}>" for k in ("k_fixup_emit", "k_fixup_apply") for t in types]
    want += ["dctz::k_fixup_scan"]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        if "k_fixup_mark<" in k["demangled"]:
            assert k.get("group_segment_fixed_size", 1 << 20) <= 16384, k
    # two waves per SIMD for the form the measurement runs (fp64 EC): 512 registers per lane of a SIMD, VGPRs and AGPRs together
    ec64 = [k for k in ks if k["demangled"].startswith("dctz::k_fixup_mark<double, 0>")]
    assert len(ec64) == 1 and ec64[0]["vgpr_count"] + ec64[0].get("agpr", 0) <= 256, ec64
