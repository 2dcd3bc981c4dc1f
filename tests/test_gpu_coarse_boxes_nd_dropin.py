"""dctz_decompress_coarse_boxes_nd (include/dctz.h) through the drop-in libraries, EC and QT builds: the boxes of one DZND
container at one factor in one call give, byte for byte, what as many dctz_decompress_coarse_box_nd calls give -- from a
container with the reference's zlib tail and from one with the DZIX chunk index, a ragged and an aligned shape of each
geometry, every factor of the geometry (factor == block edge: the DC section alone).  A flat container, a bad factor, a bad
box in the middle of the list and a bad k return -1 and leave every output unwritten; a good call follows each.

The containers and helpers are those of the other drop-in tests (tests/dropin_cases.py, tests/test_gpu_coarse_box_nd_dropin.py)."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import test_gpu_coarse_box_nd_dropin as CD
from tests import workloads as W

pytestmark = pytest.mark.gpu
EB = CD.EB
EDGE, FACTORS = CD.EDGE, CD.FACTORS
# (shape, element type): a ragged and an aligned shape of each geometry
WORK = [((45, 77), np.float32), ((64, 96), np.float64), ((13, 22, 35), np.float64), ((16, 16, 32), np.float32)]
_ids = ["45x77-float32", "64x96-float64", "13x22x35-float64", "16x16x32-float32"]


def _lib(mode):
    lib = CD._lib(mode)
    lib.dctz_decompress_coarse_boxes_nd.restype = C.c_int
    lib.dctz_decompress_coarse_boxes_nd.argtypes = [C.POINTER(D.TVar), C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                    C.POINTER(C.POINTER(D.TVar))]
    return lib


def _list(lib, z, dtype, factor, boxes, k=None):
    """(return value, the outputs): NaN-filled outputs, so that a box that was not written shows."""
    nd = len(boxes[0][0])
    outs = [np.full(max(int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)])), 1), np.nan, dtype) for lo, hi in boxes]
    tv = [D._tvar(o) for o in outs]
    ptrs = (C.POINTER(D.TVar) * max(len(tv), 1))(*[C.pointer(t) for t in tv])
    flat = lambda rows: (C.c_size_t * max(nd * len(rows), 1))(*[int(v) for r in rows for v in r])
    rc = lib.dctz_decompress_coarse_boxes_nd(C.byref(CD._zvar(z, dtype)), factor, len(boxes) if k is None else k, flat([b[0] for b in boxes]),
                                             flat([b[1] for b in boxes]), ptrs)
    return rc, outs


def _box_list(cd, K, seed):
    """The single call's boxes, one of them twice."""
    bx = CD._boxes(cd, K, seed)
    return bx + [bx[-1]]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=_ids)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_the_list_is_as_many_single_calls(mode, work, gpu_tail):
    shape, dtype = work
    lib = _lib(mode)
    nd = len(shape)
    x = W.ragged(int(np.prod(shape)), dtype, scale=37.0)
    z, _ = D._container(lib, x, EB, gpu_tail, shape)
    assert (struct.unpack_from("<I", z, 0)[0] >> 8) & 0xFF == nd
    for f in FACTORS[nd]:
        cd = tuple(-(-d // f) for d in shape)
        boxes = _box_list(cd, EDGE[nd] // f, seed=17 * f + nd)
        rc, outs = _list(lib, z, dtype, f, boxes)
        assert rc == 1, f
        for o, (lo, hi) in zip(outs, boxes):
            rc1, r = CD._box(lib, z, dtype, f, lo, hi)
            assert rc1 == 1 and o.size == r.size and np.array_equal(o.view(np.uint8), r.view(np.uint8)), (f, lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", [WORK[0], WORK[2]], ids=[_ids[0], _ids[2]])
def test_flat_containers_bad_factors_bad_boxes_and_bad_k_are_refused(mode, work):
    shape, dtype = work
    lib = _lib(mode)
    nd = len(shape)
    x = W.ragged(int(np.prod(shape)), dtype, scale=37.0)
    z, _ = D._container(lib, x, EB, False, shape)
    cd = tuple(-(-d // 2) for d in shape)
    boxes = _box_list(cd, EDGE[nd] // 2, seed=3)

    def good():
        rc, outs = _list(lib, z, dtype, 2, boxes)
        assert rc == 1
        for o, (lo, hi) in zip(outs, boxes):
            rc1, r = CD._box(lib, z, dtype, 2, lo, hi)
            assert rc1 == 1 and np.array_equal(o.view(np.uint8), r.view(np.uint8)), (lo, hi)

    def refused(rc_outs, what):
        rc, outs = rc_outs
        assert rc == -1 and all(np.isnan(o).all() for o in outs), what                 # nothing was written
        good()

    good()
    for f in (0, 1, 3, -2, 16, 128) + ((8,) if nd == 3 else ()):                        # a bad factor
        refused(_list(lib, z, dtype, f, [((0,) * nd, (1,) * nd)] * 3), f)
    mid = len(boxes) // 2
    bad = [((0,) * nd, tuple(d + 1 if i == nd - 1 else d for i, d in enumerate(cd))),   # one past the coarse extent
           ((0,) * nd, tuple(shape)),                                                  # legal in elements, not in cells
           (cd, cd)]                                                                   # lo >= hi
    for b in bad:
        bx = list(boxes)
        bx[mid] = b
        refused(_list(lib, z, dtype, 2, bx), b)
    refused(_list(lib, z, dtype, 2, boxes, k=0), "k = 0")
    refused(_list(lib, z, dtype, 2, boxes, k=-1), "k = -1")
    refused(_list(lib, z, dtype, 2, [boxes[0]], k=4097), "k = 4097")
    zf, _ = D._container(lib, x, EB, False, None)                                       # a flat container
    assert (struct.unpack_from("<I", zf, 0)[0] >> 8) & 0xFF == 0
    refused(_list(lib, zf, dtype, 2, boxes), "flat")
