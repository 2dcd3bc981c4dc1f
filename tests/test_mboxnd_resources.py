"""Register budget of the list-of-boxes decode for tiled arrays (dctz_kernels_mboxnd.hip): exactly the eight
k_decompress_mbox_nd instantiations are built, each runs without scratch and without spilled VGPRs (read from the code
object's metadata), and the list builder they share with the flat call is still built exactly once.

The kernel lives in the namespace dctz::tiled: tests/test_mbox_resources.py lists the flat call's kernels by the prefix
dctz::k_decompress_mbox and must keep seeing those eight alone."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_mboxnd_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    all_ks = kernels_of(LIB)
    ks = [k for k in all_ks if k.get("demangled", "").startswith("dctz::tiled::k_decompress_mbox_nd")]
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::tiled::k_decompress_mbox_nd<{t}, {m}, {g}>" for t in ("double", "float") for m in (0, 1) for g in (1, 2)]
    assert names == sorted(want), names
    assert not [k for k in all_ks if "k_decompress_mbox_nd" in k.get("demangled", "") and k not in ks]
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
    build = [k for k in all_ks if k.get("demangled", "").split("(")[0] == "dctz::k_boxlist_build"]
    assert len(build) == 1, [k.get("demangled") for k in all_ks if "boxlist" in k.get("demangled", "")]
