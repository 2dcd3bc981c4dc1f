"""dctz_decompress_box_nd (include/dctz.h) through the drop-in libraries, EC and QT builds: a box of what dctz_decompress
reconstructs from a DZND container (dctz_set_block_dims + dctz_compress), bit for bit, from a container with the
reference's zlib tail and from one with the DZIX chunk index (DCTZ_ZLIB_GPU=1).  On the indexed container every
compressed chunk that lies wholly beyond the prefix the box needs is zeroed first: the result does not change.  A flat
container and bad boxes are refused with -1, and a good call follows."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import workloads as W
from tests.dropin_cases import IX_MAGIC, TILE, TVar, _container, _same, _sections, _sl, _tvar

pytestmark = pytest.mark.gpu
EDGE = {2: 8, 3: 4}


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_decompress_box_nd.restype = C.c_int
    lib.dctz_decompress_box_nd.argtypes = [C.POINTER(TVar), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(TVar)]
    return lib


def _box(lib, z, dtype, lo, hi):
    ext = [max(h - l, 0) for l, h in zip(lo, hi)]
    out = np.full(max(int(np.prod(ext)), 1), np.nan, dtype)
    arr = lambda v: None if v is None else (C.c_size_t * len(v))(*v)
    rc = lib.dctz_decompress_box_nd(C.byref(_tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])), arr(lo), arr(hi), C.byref(_tvar(out)))
    return rc, out[: int(np.prod(ext))].reshape(ext) if rc == 1 else out


# (shape, element type, ten boxes): the whole array, corners, an interior box, boxes on and off block edges, one that
# ends at the last element (inside padded blocks), thin slabs along every axis, a box inside one block
WORK = [
    ((90, 130), np.float32, [((0, 0), (90, 130)), ((0, 0), (1, 1)), ((89, 129), (90, 130)), ((3, 101), (80, 125)), ((8, 16), (24, 64)),
                             ((9, 17), (23, 63)), ((60, 100), (90, 130)), ((30, 0), (31, 130)), ((0, 77), (90, 78)), ((41, 42), (46, 47))]),
    ((13, 22, 35), np.float64, [((0, 0, 0), (13, 22, 35)), ((0, 0, 0), (1, 1, 1)), ((12, 21, 34), (13, 22, 35)), ((2, 10, 5), (11, 20, 9)),
                                ((4, 8, 12), (8, 16, 24)), ((3, 7, 11), (9, 17, 25)), ((9, 15, 20), (13, 22, 35)), ((7, 0, 0), (8, 22, 35)),
                                ((0, 13, 0), (13, 14, 35)), ((5, 9, 17), (7, 11, 19))]),
]
_ids = ["90x130-float32", "13x22x35-float64"]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=_ids)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_box_is_the_slice_of_dctz_decompress(mode, work, gpu_tail):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = _container(lib, x, 1e-3, gpu_tail, dims)
    assert len(boxes) == 10
    for lo, hi in boxes:
        rc, r = _box(lib, z, dtype, lo, hi)
        assert rc == 1 and _same(r, _sl(full, dims, lo, hi)), (lo, hi)


# a larger array so that whole 16 KiB chunks of every section lie behind what an early box needs
EARLY = [
    ((300, 520), np.float32, [((0, 3), (20, 500)), ((0, 0), (1, 1)), ((40, 10), (41, 11)), ((3, 0), (4, 520)), ((1, 7), (50, 8))]),
    ((40, 44, 70), np.float64, [((0, 3, 5), (2, 40, 33)), ((0, 0, 0), (1, 1, 1)), ((5, 10, 20), (6, 11, 21)), ((3, 0, 0), (4, 44, 70)),
                                ((1, 7, 9), (9, 8, 60))]),
]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", EARLY, ids=["300x520-float32", "40x44x70-float64"])
def test_dzix_chunks_beyond_the_box_are_not_inflated(mode, work):
    dims, dtype, boxes = work
    lib = _lib(mode)
    x = W.ragged(int(np.prod(dims)), dtype, scale=37.0)
    z, full = _container(lib, x, 1e-3, True, dims)
    n, cnt, sizes, offs, end = _sections(z, dtype, mode == "qt")
    assert all(z[o + 1] == 0x5E for o in offs)          # the GPU entropy stage's mark
    magic, chunk, c0, c1, c2 = struct.unpack_from("<5I", z, end)
    assert magic == IX_MAGIC
    csz = np.frombuffer(bytes(z[end + 20:end + 20 + 2 * (c0 + c1 + c2)]), np.uint16).astype(np.int64)
    per = [csz[:c0], csz[c0:c0 + c1], csz[c0 + c1:]]
    bins = np.frombuffer(zlib.decompress(bytes(z[offs[0]:offs[0] + sizes[0]])), np.uint8)
    npos = bins.size
    flags = (bins == 255) & (np.arange(npos) % 64 != 0)
    e = EDGE[len(dims)]
    nb = [-(-d // e) for d in dims]
    for lo, hi in boxes:
        last = int(np.ravel_multi_index([(h - 1) // e for h in hi], nb))      # the last block that intersects the box
        t1 = last // 64 + 1
        need = [min(npos, TILE * t1), (last + 1) * 4, int(flags[:min(npos, TILE * t1)].sum()) * 4]
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
        rc, r = _box(lib, zz, dtype, lo, hi)
        assert rc == 1 and _same(r, _sl(full, dims, lo, hi)), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_flat_containers_and_bad_boxes_are_refused(mode):
    lib = _lib(mode)
    dims = (13, 22, 35)
    x = W.ragged(int(np.prod(dims)), np.float64, scale=37.0)
    z, full = _container(lib, x, 1e-3, False, dims)
    bad = [((0, 0, 0), (14, 22, 35)), ((0, 0, 35), (13, 22, 36)), ((5, 5, 5), (5, 6, 6)), ((6, 5, 5), (5, 6, 6))]
    for lo, hi in bad:
        assert _box(lib, z, np.float64, lo, hi)[0] == -1, (lo, hi)
    arr = lambda v: (C.c_size_t * len(v))(*v)
    out = np.zeros(8, np.float64)
    zv = _tvar(z.view(np.float64)[: z.size // 8])
    assert lib.dctz_decompress_box_nd(C.byref(zv), None, arr((1, 1, 1)), C.byref(_tvar(out))) == -1
    assert lib.dctz_decompress_box_nd(C.byref(zv), arr((0, 0, 0)), None, C.byref(_tvar(out))) == -1
    zf, _ = _container(lib, x, 1e-3, False)        # flat blocks
    assert (struct.unpack_from("<I", zf, 0)[0] >> 8) & 0xFF == 0
    assert _box(lib, zf, np.float64, (0, 0, 0), (1, 1, 1))[0] == -1
    # and the library still decodes a box of the tiled container afterwards
    rc, r = _box(lib, z, np.float64, (1, 2, 3), (12, 20, 30))
    assert rc == 1 and _same(r, _sl(full, dims, (1, 2, 3), (12, 20, 30)))
