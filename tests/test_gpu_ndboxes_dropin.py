"""dctz_decompress_boxes_nd (include/dctz.h) through the drop-in libraries, EC and QT builds: six boxes of one DZND
container (dctz_set_block_dims + dctz_compress) in one call give the bytes of six dctz_decompress_box_nd calls, from a
container with the reference's zlib tail and from one with the DZIX chunk index.  On the indexed container every compressed
chunk that lies wholly beyond what the LAST intersecting block of any box needs is zeroed first: the result does not
change.  A flat container, a bad box anywhere in the list and a bad k are refused with dctz_decompress_box_nd's -1, and
dctz_decompress_boxes keeps refusing the DZND container.

The containers and helpers are those of the single-box drop-in tests (tests/dropin_cases.py, tests/test_gpu_ndbox_dropin.py)."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import test_gpu_ndbox_dropin as ND
from tests import workloads as W

pytestmark = pytest.mark.gpu
TILE = D.TILE
EDGE = ND.EDGE

# (shape, element type, six boxes): overlapping, nested, one repeated, one that ends at the last element
WORK = [
    ((90, 130), np.float32, [((0, 0), (90, 130)), ((0, 0), (1, 1)), ((3, 101), (80, 125)), ((60, 100), (90, 130)), ((9, 105), (23, 120)),
                             ((3, 101), (80, 125))]),
    ((13, 22, 35), np.float64, [((0, 0, 0), (13, 22, 35)), ((0, 0, 0), (1, 1, 1)), ((2, 10, 5), (11, 20, 9)), ((9, 15, 20), (13, 22, 35)),
                                ((7, 0, 0), (8, 22, 35)), ((2, 10, 5), (11, 20, 9))]),
]
_ids = ["90x130-float32", "13x22x35-float64"]
# boxes that all end early in the array: whole 16 KiB chunks of every section lie behind what the list needs
EARLY = [
    ((300, 520), np.float32, [((0, 3), (20, 500)), ((0, 0), (1, 1)), ((40, 10), (41, 11)), ((3, 0), (4, 520)), ((1, 7), (50, 8)),
                              ((0, 3), (20, 500))]),
    ((40, 44, 70), np.float64, [((0, 3, 5), (2, 40, 33)), ((0, 0, 0), (1, 1, 1)), ((5, 10, 20), (6, 11, 21)), ((3, 0, 0), (4, 44, 70)),
                                ((1, 7, 9), (9, 8, 60)), ((0, 3, 5), (2, 40, 33))]),
]


def _lib(mode):
    lib = ND._lib(mode)
    lib.dctz_decompress_boxes_nd.restype = C.c_int
    lib.dctz_decompress_boxes_nd.argtypes = [C.POINTER(D.TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                             C.POINTER(C.POINTER(D.TVar))]
    lib.dctz_decompress_boxes.restype = C.c_int
    lib.dctz_decompress_boxes.argtypes = [C.POINTER(D.TVar), C.c_int, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.POINTER(C.POINTER(D.TVar))]
    return lib


def _args(z, dtype, boxes):
    nd = len(boxes[0][0])
    outs = [np.full(max(int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)])), 1), np.nan, dtype) for lo, hi in boxes]
    tv = [D._tvar(o) for o in outs]
    ptrs = (C.POINTER(D.TVar) * max(len(tv), 1))(*[C.pointer(t) for t in tv])
    flat = lambda rows: (C.c_size_t * max(nd * len(rows), 1))(*[int(v) for r in rows for v in r])
    zv = D._tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])
    return zv, flat([b[0] for b in boxes]), flat([b[1] for b in boxes]), ptrs, outs, tv


def _boxes(lib, z, dtype, boxes, k=None):
    """(return value, the outputs): NaN-filled outputs, so that a box that was not written shows."""
    zv, lo, hi, ptrs, outs, tv = _args(z, dtype, boxes)
    rc = lib.dctz_decompress_boxes_nd(C.byref(zv), len(boxes) if k is None else k, lo, hi, ptrs)
    return rc, outs


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=_ids)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_six_boxes_are_six_single_calls(mode, work, gpu_tail):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, gpu_tail, dims)
    assert len(boxes) == 6
    rc, outs = _boxes(lib, z, dtype, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        rc1, r = ND._box(lib, z, dtype, lo, hi)
        assert rc1 == 1 and D._same(o.reshape(r.shape), r), (lo, hi)
        assert D._same(r, D._sl(full, dims, lo, hi))


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", EARLY, ids=["300x520-float32", "40x44x70-float64"])
def test_dzix_chunks_beyond_the_union_span_are_not_inflated(mode, work):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, True, dims)
    n, cnt, sizes, offs, end = D._sections(z, dtype, mode == "qt")
    assert all(z[o + 1] == 0x5E for o in offs)          # the GPU entropy stage's mark
    magic, chunk, c0, c1, c2 = struct.unpack_from("<5I", z, end)
    assert magic == D.IX_MAGIC
    csz = np.frombuffer(bytes(z[end + 20:end + 20 + 2 * (c0 + c1 + c2)]), np.uint16).astype(np.int64)
    per = [csz[:c0], csz[c0:c0 + c1], csz[c0 + c1:]]
    bins = np.frombuffer(zlib.decompress(bytes(z[offs[0]:offs[0] + sizes[0]])), np.uint8)
    npos = bins.size
    flags = (bins == 255) & (np.arange(npos) % 64 != 0)
    e = EDGE[len(dims)]
    nb = [-(-d // e) for d in dims]
    last = max(int(np.ravel_multi_index([(h - 1) // e for h in hi], nb)) for lo, hi in boxes)    # the last block any box intersects
    t1 = last // 64 + 1
    need = [min(npos, TILE * t1), (last + 1) * 4, int(flags[:min(npos, TILE * t1)].sum()) * 4]
    zz = z.copy()
    zeroed = 0
    for i in range(3):
        off = offs[i] + 2
        for j, s in enumerate(per[i]):
            if j * chunk >= need[i]:                      # wholly beyond what the list needs
                zz[off:off + s] = 0
                zeroed += 1
            off += s
    assert zeroed > 0
    rc, outs = _boxes(lib, zz, dtype, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        want = D._sl(full, dims, lo, hi)
        assert D._same(o.reshape(want.shape), want), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_flat_containers_bad_boxes_and_bad_k_are_refused(mode):
    lib = _lib(mode)
    dims, dtype, boxes = WORK[1]
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, False, dims)
    for j, bad in ((0, ((0, 0, 0), (14, 22, 35))), (3, ((5, 5, 5), (5, 6, 6))), (5, ((0, 0, 35), (13, 22, 36)))):
        bx = list(boxes)
        bx[j] = bad
        rc, outs = _boxes(lib, z, dtype, bx)
        assert rc == -1 and all(np.isnan(o).all() for o in outs), (j, bad)          # nothing was written
    assert _boxes(lib, z, dtype, boxes, k=0)[0] == -1
    assert _boxes(lib, z, dtype, boxes, k=4097)[0] == -1
    zf, _ = D._container(lib, x, 1e-3, False)            # flat blocks
    assert (struct.unpack_from("<I", zf, 0)[0] >> 8) & 0xFF == 0
    assert _boxes(lib, zf, dtype, boxes)[0] == -1
    # dctz_decompress_boxes keeps refusing the DZND container
    zv, lo, hi, ptrs, outs, tv = _args(z, dtype, boxes)
    assert lib.dctz_decompress_boxes(C.byref(zv), 3, (C.c_size_t * 3)(*dims), len(boxes), lo, hi, ptrs) == -1
    assert all(np.isnan(o).all() for o in outs)
    # and the library still decodes a list of the tiled container afterwards
    rc, outs = _boxes(lib, z, dtype, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        want = D._sl(full, dims, lo, hi)
        assert D._same(o.reshape(want.shape), want), (lo, hi)
