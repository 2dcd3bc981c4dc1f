"""dctz_decompress_range (include/dctz.h) through the drop-in libraries, EC and QT builds: elements [lo, hi) of what
dctz_decompress reconstructs, bit for bit, from a container with the reference's zlib tail and from one with the DZIX
chunk index (DCTZ_ZLIB_GPU=1).  On the indexed container, every compressed chunk that lies wholly beyond what the range
needs is zeroed first: the result does not change, so those chunks are not inflated.  A DZND container and bad ranges
are refused with -1."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import workloads as W
from tests.dropin_cases import IX_MAGIC, TILE, TVar, _container, _sections, _tvar

pytestmark = pytest.mark.gpu


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_decompress_range.restype = C.c_int
    lib.dctz_decompress_range.argtypes = [C.POINTER(TVar), C.c_size_t, C.c_size_t, C.POINTER(TVar)]
    return lib


def _range(lib, z, dtype, lo, hi):
    out = np.full(max(hi - lo, 1), np.nan, dtype)
    rc = lib.dctz_decompress_range(C.byref(_tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])), lo, hi, C.byref(_tvar(out)))
    return rc, out[: hi - lo]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


N = 64 * 20000 + 37                                    # 1.28 M elements: many 4096-element tiles, a short last block
RANGES = [(0, 1), (0, N), (N - 1, N), (5, 9), (TILE - 3, TILE + 70), (100, 5000), (N // 2, N // 2 + (1 << 16) + 3),
          (N - 45, N), (N - 64 * 100 - 7, N), (7 * TILE, 9 * TILE), (123457, 123458)]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_range_is_the_slice_of_dctz_decompress(mode, dtype, gpu_tail):
    lib = _lib(mode)
    x = W.ragged(N, dtype, scale=37.0)
    z, full = _container(lib, x, 1e-3, gpu_tail)
    for lo, hi in RANGES:
        rc, r = _range(lib, z, dtype, lo, hi)
        assert rc == 1 and _same(r, full[lo:hi]), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dzix_chunks_beyond_the_range_are_not_inflated(mode, dtype):
    lib = _lib(mode)
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
    for lo, hi in [(100, 5000), (0, 1), (3 * TILE + 5, 6 * TILE - 1), (N // 3, N // 3 + 20000)]:
        t1 = -(-hi // TILE)
        need = [min(n, TILE * t1), -(-hi // 64) * 4, int(flags[:min(n, TILE * t1)].sum()) * 4]
        zz = z.copy()
        zeroed = 0
        for i in range(3):
            off = offs[i] + 2
            for j, s in enumerate(per[i]):
                if j * chunk >= need[i]:                  # wholly beyond what the range needs
                    zz[off:off + s] = 0
                    zeroed += 1
                off += s
        assert zeroed > 0
        rc, r = _range(lib, zz, dtype, lo, hi)
        assert rc == 1 and _same(r, full[lo:hi]), (lo, hi)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_dznd_and_bad_ranges_are_refused(mode):
    lib = _lib(mode)
    x = W.ragged(N, np.float64, scale=37.0)
    z, full = _container(lib, x, 1e-3, False)
    for lo, hi in [(5, 5), (6, 5), (0, N + 1), (N, N + 1)]:
        assert _range(lib, z, np.float64, lo, hi)[0] == -1, (lo, hi)
    shape = (96, 80)
    y = W.ragged(shape[0] * shape[1], np.float64, scale=37.0)
    assert lib.dctz_set_block_dims(2, (C.c_size_t * 2)(*shape)) == 0
    zn, _ = _container(lib, y, 1e-3, False)
    assert (struct.unpack_from("<I", zn, 0)[0] >> 8) & 0xFF == 2
    assert _range(lib, zn, np.float64, 0, 10)[0] == -1
    # and the library still decodes a flat container afterwards
    rc, r = _range(lib, z, np.float64, 10, 5000)
    assert rc == 1 and _same(r, full[10:5000])
