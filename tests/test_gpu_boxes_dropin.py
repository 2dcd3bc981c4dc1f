"""dctz_decompress_boxes (include/dctz.h) through the drop-in libraries, EC and QT builds: six boxes of one container in one
call give the bytes of six dctz_decompress_box calls, from a container with the reference's zlib tail and from one with the
DZIX chunk index.  On the indexed container every compressed chunk that lies wholly beyond what the LAST element of any
box needs is zeroed first: the result does not change.  A DZND container, a bad box anywhere in the list and a bad k are
refused with dctz_decompress_box's -1.

The containers and helpers are those of the single-box drop-in test, from tests/dropin_cases.py."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import workloads as W

pytestmark = pytest.mark.gpu
TILE = D.TILE

# (shape, element type, six boxes): overlapping, nested, one repeated, one that ends at the last element
WORK = [
    ((33, 65, 67), np.float64, [((0, 0, 0), (33, 65, 67)), ((0, 0, 0), (1, 1, 1)), ((2, 10, 5), (30, 20, 9)), ((30, 60, 1), (33, 65, 67)),
                                ((7, 0, 0), (8, 65, 67)), ((2, 10, 5), (30, 20, 9))]),
    ((4, 40, 512), np.float32, [((1, 3, 100), (3, 5, 200)), ((0, 39, 0), (4, 40, 512)), ((0, 0, 5), (4, 1, 6)), ((3, 39, 511), (4, 40, 512)),
                                ((0, 0, 0), (4, 40, 512)), ((2, 4, 150), (3, 5, 160))]),
]
# boxes that all end early in the array: whole 16 KiB chunks of every section lie behind what the list needs
EARLY = [
    ((33, 65, 67), np.float64, [((0, 3, 5), (2, 60, 33)), ((0, 0, 0), (1, 1, 1)), ((5, 10, 20), (6, 11, 21)), ((3, 0, 0), (4, 65, 67)),
                                ((1, 7, 9), (9, 8, 60)), ((0, 3, 5), (2, 60, 33))]),
    ((4, 40, 512), np.float32, [((0, 3, 5), (1, 30, 33)), ((0, 0, 0), (1, 1, 1)), ((0, 10, 20), (2, 11, 21)), ((1, 0, 0), (2, 3, 512)),
                                ((0, 7, 9), (1, 8, 60)), ((1, 0, 100), (2, 2, 300))]),
]
_ids = ["33x65x67-float64", "4x40x512-float32"]


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_decompress_boxes.restype = C.c_int
    lib.dctz_decompress_boxes.argtypes = [C.POINTER(D.TVar), C.c_int, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.POINTER(C.POINTER(D.TVar))]
    return lib


def _boxes(lib, z, dtype, dims, boxes, k=None):
    """(return value, the outputs): NaN-filled outputs, so that a box that was not written shows."""
    nd = len(dims)
    outs = [np.full(max(int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)])), 1), np.nan, dtype) for lo, hi in boxes]
    tv = [D._tvar(o) for o in outs]
    ptrs = (C.POINTER(D.TVar) * max(len(tv), 1))(*[C.pointer(t) for t in tv])
    flat = lambda rows: (C.c_size_t * max(nd * len(rows), 1))(*[int(v) for r in rows for v in r])
    zv = D._tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])
    rc = lib.dctz_decompress_boxes(C.byref(zv), nd, (C.c_size_t * nd)(*dims), len(boxes) if k is None else k,
                                   flat([b[0] for b in boxes]), flat([b[1] for b in boxes]), ptrs)
    return rc, outs


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=_ids)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_six_boxes_are_six_single_calls(mode, work, gpu_tail):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, gpu_tail)
    rc, outs = _boxes(lib, z, dtype, dims, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        rc1, r = D._box(lib, z, dtype, dims, lo, hi)
        assert rc1 == 1 and D._same(o.reshape(r.shape), r), (lo, hi)
        assert D._same(r, D._sl(full, dims, lo, hi))


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", EARLY, ids=_ids)
def test_dzix_chunks_beyond_the_union_span_are_not_inflated(mode, work):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, True)
    n, cnt, sizes, offs, end = D._sections(z, dtype, mode == "qt")
    assert all(z[o + 1] == 0x5E for o in offs)          # the GPU entropy stage's mark
    magic, chunk, c0, c1, c2 = struct.unpack_from("<5I", z, end)
    assert magic == D.IX_MAGIC
    csz = np.frombuffer(bytes(z[end + 20:end + 20 + 2 * (c0 + c1 + c2)]), np.uint16).astype(np.int64)
    per = [csz[:c0], csz[c0:c0 + c1], csz[c0 + c1:]]
    bins = np.frombuffer(zlib.decompress(bytes(z[offs[0]:offs[0] + sizes[0]])), np.uint8)
    flags = (bins == 255) & (np.arange(n) % 64 != 0)
    last = max(int(np.ravel_multi_index([h - 1 for h in hi], dims)) for lo, hi in boxes)
    t1 = last // TILE + 1
    need = [min(n, TILE * t1), -(-(last + 1) // 64) * 4, int(flags[:min(n, TILE * t1)].sum()) * 4]
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
    rc, outs = _boxes(lib, zz, dtype, dims, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        want = D._sl(full, dims, lo, hi)
        assert D._same(o.reshape(want.shape), want), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_dznd_bad_boxes_and_bad_k_are_refused(mode):
    lib = _lib(mode)
    dims, dtype, boxes = WORK[0]
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = D._container(lib, x, 1e-3, False)
    for j, bad in ((0, ((0, 0, 0), (34, 65, 67))), (3, ((5, 5, 5), (5, 6, 6))), (5, ((0, 0, 67), (33, 65, 68)))):
        bx = list(boxes)
        bx[j] = bad
        rc, outs = _boxes(lib, z, dtype, dims, bx)
        assert rc == -1 and all(np.isnan(o).all() for o in outs), (j, bad)          # nothing was written
    assert _boxes(lib, z, dtype, dims, boxes, k=0)[0] == -1
    assert _boxes(lib, z, dtype, dims, boxes, k=4097)[0] == -1
    assert _boxes(lib, z, dtype, (33, 65, 66), boxes[1:2])[0] == -1                 # prod dims != N
    shape = (96, 80)
    y = W.ragged(shape[0] * shape[1], np.float64, scale=37.0)
    assert lib.dctz_set_block_dims(2, (C.c_size_t * 2)(*shape)) == 0
    zn, _ = D._container(lib, y, 1e-3, False)
    assert (struct.unpack_from("<I", zn, 0)[0] >> 8) & 0xFF == 2
    assert D._box(lib, zn, np.float64, shape, (0, 0), (10, 10))[0] == -1
    assert _boxes(lib, zn, np.float64, shape, [((0, 0), (10, 10)), ((5, 5), (6, 6))])[0] == -1
    # and the library still decodes a list of a flat container afterwards
    rc, outs = _boxes(lib, z, dtype, dims, boxes)
    assert rc == 1
    for o, (lo, hi) in zip(outs, boxes):
        want = D._sl(full, dims, lo, hi)
        assert D._same(o.reshape(want.shape), want), (lo, hi)
