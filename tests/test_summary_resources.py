"""Register budget of the tile summaries (dctz_kernels_summary.hip): exactly the intended instantiations are built -- T x MODE x
REF of k_tile_summary and of k_tile_summary_rem, and k_tile_summary_final -- and each runs without scratch and without
spilled VGPRs (read from the code object's metadata)."""
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


def test_summary_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    ks = [k for k in kernels_of(LIB) if k.get("demangled", "").startswith("dctz::k_tile_summary")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    types, modes, refs = ("double", "float"), (0, 1), ("false", "true")
    want = [f"dctz::{k}<{t}, {m}, {r}>" for k in ("k_tile_summary", "k_tile_summary_rem") for t in types for m in modes for r in refs]
    want += ["dctz::k_tile_summary_final"]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
