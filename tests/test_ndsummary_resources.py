"""Budget of the tile summaries for tiled arrays (dctz_kernels_ndsummary.hip): exactly the sixteen instantiations of k_ndsummary
are built -- T x MODE x GEOM x REF --, none has scratch or a spilled VGPR, with the original the LDS is the tile image of the
box decoder and the correction list (NdImage<T, GEOM>::BYTES), without it no more than the flat summary's
(SummaryLds<T>::BYTES, at most 16 KiB: two waves per SIMD).  Read from the code object's metadata."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib", "libdctzhip.so")
TILE_BLKS = 64
SUMMARY_LDS = 16384                   # SummaryLds<T>::BYTES is at most this: half an fp64 tile, or a dense tile's staged coefficients (63 * 64 * 4)


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


def test_exactly_sixteen_kernels_without_scratch():
    ks = _kernels("dctz::k_ndsummary")
    names = sorted(k["demangled"].split("(")[0] for k in ks)
    want = [f"dctz::k_ndsummary<{t}, {m}, {g}, {r}>" for t in ("double", "float") for m in (0, 1) for g in (1, 2) for r in ("false", "true")]
    assert len(want) == 16 and names == sorted(want), names
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k


def test_lds_is_the_image_with_the_original_and_the_staging_without():
    flat = {k["demangled"].split("(")[0]: k["group_segment_fixed_size"] for k in _kernels("dctz::k_tile_summary<")}
    mark = {k["demangled"].split("(")[0].split("k_ndfix_mark")[1]: k["group_segment_fixed_size"] for k in _kernels("dctz::k_ndfix_mark")}
    assert len(mark) == 8
    for k in _kernels("dctz::k_ndsummary"):
        inst = k["demangled"].split("(")[0].split("k_ndsummary")[1]             # "<double, 0, 1, true>"
        t, m, g, r = [v.strip() for v in inst.strip("<>").split(",")]
        if r == "true":
            assert k["group_segment_fixed_size"] == _image_bytes(t, int(g)) == mark[f"<{t}, {m}, {g}>"], k
        else:
            # SummaryLds<T>::BYTES is what the flat kernel of the same type and mode allocates
            assert 63 * 64 * 4 <= k["group_segment_fixed_size"] <= flat[f"dctz::k_tile_summary<{t}, {m}, false>"] <= SUMMARY_LDS, (k, flat)
