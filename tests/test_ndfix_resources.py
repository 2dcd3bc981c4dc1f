"""Budget of the correction list for tiled arrays (dctz_kernels_ndfix.hip): exactly the intended instantiations of k_ndfix_mark,
k_ndfix_emit and k_ndfix_apply are built, none has scratch or a spilled VGPR, and the mark kernel's LDS is the tile image of
the box decoder it is built from (NdImage<T, GEOM>::BYTES; read from the code object's metadata)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")
TILE_BLKS = 64


@pytest.fixture(scope="module", autouse=True)
def built():
    """A missing library is built, as tests/test_abi_cpu.py does; one that does not build fails the test."""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def _image_bytes(t, g):
    """NdImage<T, GEOM>::BYTES (dctz_nd_image.h): 64 blocks at a stride of 68 elements in 3-D, 70 (fp64) / 72 (fp32) in 2-D."""
    stride = 68 if g == 2 else (70 if t == "double" else 72)
    return TILE_BLKS * stride * (8 if t == "double" else 4)


def _kernels(prefix):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    return [k for k in kernels_of(LIB) if k.get("demangled", "").startswith(prefix)]


def test_exactly_the_intended_kernels_without_scratch():
    ks = _kernels("dctz::k_ndfix")
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::k_ndfix_mark<{t}, {m}, {g}>" for t in ("double", "float") for m in (0, 1) for g in (1, 2)]
    want += [f"dctz::k_ndfix_{k}<{t}, {g}>" for k in ("emit", "apply") for t in ("double", "float") for g in (1, 2)]
    assert names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k


def test_mark_lds_is_the_box_decoders_image():
    box = {k["demangled"].split("(")[0].split("k_decompress_ndbox")[1]: k for k in _kernels("dctz::k_decompress_ndbox")}
    assert len(box) == 8
    for k in _kernels("dctz::k_ndfix_mark"):
        inst = k["demangled"].split("(")[0].split("k_ndfix_mark")[1]           # "<double, 0, 1>"
        t, _, g = [v.strip() for v in inst.strip("<>").split(",")]
        assert k["group_segment_fixed_size"] == _image_bytes(t, int(g)) == box[inst]["group_segment_fixed_size"], k
    for k in _kernels("dctz::k_ndfix_emit") + _kernels("dctz::k_ndfix_apply"):
        assert k.get("group_segment_fixed_size", 0) == 0, k

