"""dctz_decompress_box (include/dctz.h) through the drop-in libraries, EC and QT builds: a box of what dctz_decompress
reconstructs, bit for bit, from a container with the reference's zlib tail and from one with the DZIX chunk index
(DCTZ_ZLIB_GPU=1, read at every dctz_compress call).  On the indexed container every compressed chunk that lies wholly
beyond what the box's last tile needs is zeroed first: the result does not change.  A box outside the shape, a shape
whose product is not the header's count and a DZND container are refused with -1."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import workloads as W
from tests.dropin_cases import IX_MAGIC, TILE, _box, _container, _lib, _same, _sections, _sl

pytestmark = pytest.mark.gpu

# (shape, element type, five boxes): the whole array, a corner, an interior box, one that ends at the last element (the
# short block inside), a thin slab
WORK = [
    ((33, 65, 67), np.float64, [((0, 0, 0), (33, 65, 67)), ((0, 0, 0), (1, 1, 1)), ((2, 10, 5), (30, 20, 9)), ((30, 60, 1), (33, 65, 67)),
                                ((7, 0, 0), (8, 65, 67))]),
    ((130, 1000), np.float32, [((0, 0), (130, 1000)), ((129, 999), (130, 1000)), ((3, 101), (120, 140)), ((100, 977), (130, 1000)),
                               ((0, 500), (130, 501))]),
]
_ids = ["33x65x67-float64", "130x1000-float32"]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=_ids)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_box_is_the_slice_of_dctz_decompress(mode, work, gpu_tail):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = _container(lib, x, 1e-3, gpu_tail)
    for lo, hi in boxes:
        rc, r = _box(lib, z, dtype, dims, lo, hi)
        assert rc == 1 and _same(r, _sl(full, dims, lo, hi)), (lo, hi)


# boxes that end early in the array: whole 16 KiB chunks of every section lie behind what they need
EARLY = [
    ((33, 65, 67), np.float64, [((0, 3, 5), (2, 60, 33)), ((0, 0, 0), (1, 1, 1)), ((5, 10, 20), (6, 11, 21)), ((3, 0, 0), (4, 65, 67)),
                                ((1, 7, 9), (9, 8, 60))]),
    ((130, 1000), np.float32, [((0, 3), (20, 500)), ((0, 0), (1, 1)), ((40, 10), (41, 11)), ((3, 0), (4, 1000)), ((1, 7), (50, 8))]),
]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", EARLY, ids=_ids)
def test_dzix_chunks_beyond_the_box_are_not_inflated(mode, work):
    DZ_DIMS, dtype, DZ_BOXES = work
    lib = _lib(mode)
    N = int(np.prod(DZ_DIMS))
    x = W.ragged(N, dtype, scale=37.0)
    z, full = _container(lib, x, 1e-3, True)
    n, cnt, sizes, offs, end = _sections(z, dtype, mode == "qt")
    assert all(z[o + 1] == 0x5E for o in offs)          # the GPU entropy stage's mark
    magic, chunk, c0, c1, c2 = struct.unpack_from("<5I", z, end)
    assert magic == IX_MAGIC
    csz = np.frombuffer(bytes(z[end + 20:end + 20 + 2 * (c0 + c1 + c2)]), np.uint16).astype(np.int64)
    per = [csz[:c0], csz[c0:c0 + c1], csz[c0 + c1:]]
    bins = np.frombuffer(zlib.decompress(bytes(z[offs[0]:offs[0] + sizes[0]])), np.uint8)
    flags = (bins == 255) & (np.arange(n) % 64 != 0)
    for lo, hi in DZ_BOXES:
        last = int(np.ravel_multi_index([h - 1 for h in hi], DZ_DIMS))
        t1 = last // TILE + 1
        need = [min(n, TILE * t1), -(-(last + 1) // 64) * 4, int(flags[:min(n, TILE * t1)].sum()) * 4]
        zz = z.copy()
        zeroed = 0
        for i in range(3):
            off = offs[i] + 2
            for j, s in enumerate(per[i]):
                if j * chunk >= need[i]:                  # wholly beyond what the box needs
                    zz[off:off + s] = 0
                    zeroed += 1
                off += s
        assert zeroed > 0
        rc, r = _box(lib, zz, dtype, DZ_DIMS, lo, hi)
        assert rc == 1 and _same(r, _sl(full, DZ_DIMS, lo, hi)), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_dznd_and_bad_boxes_are_refused(mode):
    lib = _lib(mode)
    dims = (33, 65, 67)
    x = W.ragged(int(np.prod(dims)), np.float64, scale=37.0)
    z, full = _container(lib, x, 1e-3, False)
    bad = [(dims, (0, 0, 0), (34, 65, 67)), (dims, (0, 0, 67), (33, 65, 68)), (dims, (5, 5, 5), (5, 6, 6)), (dims, (6, 5, 5), (5, 6, 6)),
           ((33, 65, 66), (0, 0, 0), (1, 1, 1)), ((33, 65, 67, 2), (0, 0, 0, 0), (1, 1, 1, 1)), ((33 * 65 * 67 + 1,), (0,), (1,)),
           ((1, 1, 1, 1) + dims[:1], (0,) * 5, (1,) * 5)]
    for d, lo, hi in bad:
        assert _box(lib, z, np.float64, d, lo, hi)[0] == -1, (d, lo, hi)
    shape = (96, 80)
    y = W.ragged(shape[0] * shape[1], np.float64, scale=37.0)
    assert lib.dctz_set_block_dims(2, (C.c_size_t * 2)(*shape)) == 0
    zn, _ = _container(lib, y, 1e-3, False)
    assert (struct.unpack_from("<I", zn, 0)[0] >> 8) & 0xFF == 2
    assert _box(lib, zn, np.float64, shape, (0, 0), (10, 10))[0] == -1
    # and the library still decodes a box of a flat container afterwards
    rc, r = _box(lib, z, np.float64, dims, (1, 2, 3), (20, 30, 40))
    assert rc == 1 and _same(r, _sl(full, dims, (1, 2, 3), (20, 30, 40)))
