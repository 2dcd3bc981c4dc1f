"""What the drop-in readers that do not decode the whole array share (include/dctz.h: dctz_decompress_range, _box, _boxes,
_box_nd, _coarse, dctz_tile_summary, dctz_fixup_build), EC and QT builds: the way from a container's sections to the device.
A container whose bin ids flag more AC_exact words than its header counts is refused by every one of them with -1 and
nothing is written; after a good call the four stage times of dctz_last_stage_times are disjoint parts of the total, from a
container with the reference's zlib tail and from one with the DZIX chunk index (DCTZ_ZLIB_GPU=1)."""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import dropin_cases as D
from tests import workloads as W

pytestmark = pytest.mark.gpu
EB = 1e-3
N = 3 * D.TILE + 37                                      # three full tiles and a short last block
DIMS = (25, 493)                                         # ... seen as a 2-D array by the box calls
SHAPE = (20, 13)                                         # 8 x 8 tiles with ragged edges, one stream tile
SENTINEL = 12345


class StageTimes(C.Structure):   # dctz.h: dctz_stage_times
    _fields_ = [(f, C.c_double) for f in ("h2d_s", "gpu_s", "d2h_s", "zlib_s", "total_s")]


def _lib(mode):
    lib = D._lib(mode)
    T, S = C.POINTER(D.TVar), C.POINTER(C.c_size_t)
    for name, args in (("dctz_decompress_range", [T, C.c_size_t, C.c_size_t, T]),
                       ("dctz_decompress_boxes", [T, C.c_int, S, C.c_int, S, S, C.POINTER(T)]),
                       ("dctz_decompress_box_nd", [T, S, S, T]),
                       ("dctz_decompress_coarse", [T, C.c_int, T]),
                       ("dctz_tile_summary", [T, T, C.c_int, C.c_void_p, C.c_void_p]),
                       ("dctz_fixup_build", [T, T, C.c_int, C.c_double, C.POINTER(C.c_void_p), S])):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = args
    lib.dctz_last_stage_times.restype = None
    lib.dctz_last_stage_times.argtypes = [C.POINTER(StageTimes)]
    return lib


@functools.lru_cache(maxsize=None)
def _containers(mode, gpu_tail):
    """(the flat array, its container, the tiled array, its container), made once; nobody writes to them."""
    lib = _lib(mode)
    assert N == DIMS[0] * DIMS[1]
    x = W.ragged(N, np.float64, scale=37.0)
    y = W.ragged(SHAPE[0] * SHAPE[1], np.float64, scale=37.0)
    z, _ = D._container(lib, x, EB, gpu_tail)
    zn, _ = D._container(lib, y, EB, gpu_tail, SHAPE)
    for c in (z, zn):
        assert (c[56 + 1] == 0x5E) == bool(gpu_tail)     # the GPU entropy stage's mark
        assert struct.unpack_from("<I", c, 16)[0] >= 1   # tot_AC_exact_count
    return x, z, y, zn


def _arr(v):
    return (C.c_size_t * len(v))(*v)


def _readers(lib, x, z, tiled):
    """[(name, call)]: call() runs one reader over the whole array into fresh sentinel-filled outputs and returns (return
    value, whether every output still holds its sentinel)."""
    zv = D._tvar(z.view(np.float64)[: z.size // 8])
    nan_out = lambda m: np.full(m, np.nan, np.float64)
    untouched = lambda o: bool(np.isnan(o).all())

    def range_():
        o = nan_out(N)
        return lib.dctz_decompress_range(C.byref(zv), 0, N, C.byref(D._tvar(o))), untouched(o)

    def box():
        o = nan_out(N)
        return lib.dctz_decompress_box(C.byref(zv), 2, _arr(DIMS), _arr((0, 0)), _arr(DIMS), C.byref(D._tvar(o))), untouched(o)

    def boxes():
        o = nan_out(N)
        tv = D._tvar(o)
        ptrs = (C.POINTER(D.TVar) * 1)(C.pointer(tv))
        return lib.dctz_decompress_boxes(C.byref(zv), 2, _arr(DIMS), 1, _arr((0, 0)), _arr(DIMS), ptrs), untouched(o)

    def box_nd():
        o = nan_out(x.size)
        return lib.dctz_decompress_box_nd(C.byref(zv), _arr((0, 0)), _arr(SHAPE), C.byref(D._tvar(o))), untouched(o)

    def coarse():
        o = nan_out(int(np.prod([-(-d // 2) for d in SHAPE])) if tiled else -(-N // 2))
        return lib.dctz_decompress_coarse(C.byref(zv), 2, C.byref(D._tvar(o))), untouched(o)

    def tile_summary():
        tiles = -(-N // D.TILE)
        recs = np.full((tiles, 8), np.nan)
        total = np.full(C.sizeof(H.TileSummary) // 8, np.nan)
        ref = x.copy()
        rc = lib.dctz_tile_summary(C.byref(zv), C.byref(D._tvar(ref)), N, recs.ctypes.data_as(C.c_void_p), total.ctypes.data_as(C.c_void_p))
        return rc, untouched(recs) and untouched(total)

    def fixup_build():
        blob, nbytes = C.c_void_p(), C.c_size_t(SENTINEL)
        ref = x.copy()
        rc = lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), x.size, 0.25 * EB, C.byref(blob), C.byref(nbytes))
        same = blob.value is None and nbytes.value == SENTINEL
        if blob.value is not None:
            libc = C.CDLL(None)
            libc.free.argtypes = [C.c_void_p]
            libc.free(blob)
        return rc, same

    calls = [box_nd, coarse, fixup_build] if tiled else [range_, box, boxes, coarse, tile_summary, fixup_build]
    return [(f.__name__, f) for f in calls]


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_streams_that_disagree_are_refused_and_nothing_is_written(mode):
    lib = _lib(mode)
    x, z, y, zn = _containers(mode, False)
    for a, c, tiled in ((x, z, False), (y, zn, True)):
        bad = c.copy()
        cnt = struct.unpack_from("<I", bad, 16)[0]
        struct.pack_into("<I", bad, 16, cnt - 1)         # the bin ids now flag one word more than the header counts
        for name, call in _readers(lib, a, bad, tiled):
            assert call() == (-1, True), (name, tiled)
        for name, call in _readers(lib, a, c, tiled):    # and the undamaged container is served afterwards
            assert call() == (1, False), (name, tiled)


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_stage_times_are_disjoint_parts_of_the_total(mode, gpu_tail):
    lib = _lib(mode)
    x, z, y, zn = _containers(mode, gpu_tail)
    for a, c, tiled in ((x, z, False), (y, zn, True)):
        for name, call in _readers(lib, a, c, tiled):
            assert call() == (1, False), (name, tiled)
            t = StageTimes(*([math.nan] * 5))
            lib.dctz_last_stage_times(C.byref(t))
            parts = [t.zlib_s, t.h2d_s, t.gpu_s, t.d2h_s]
            print(name, "tiled" if tiled else "flat", parts, t.total_s)
            assert all(math.isfinite(v) and v >= 0.0 for v in parts + [t.total_s]), (name, tiled, parts, t.total_s)
            assert t.total_s > 0.0, (name, tiled)
            # four disjoint intervals inside the call; the millisecond is gettimeofday's resolution, with room
            assert sum(parts) <= t.total_s + 1e-3, (name, tiled, parts, t.total_s)
