"""dctz_decompress_coarse_box_nd (include/dctz.h) through the drop-in libraries, EC and QT builds: the result is, byte for byte,
the slice of what dctz_decompress_coarse returns for the same container and factor.  A flat container, a bad factor and a
box that is not inside the coarse extents return -1, and a good call follows each."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import workloads as W
from tests.dropin_cases import TVar, _tvar

pytestmark = pytest.mark.gpu
EB = 1e-3
EDGE = {2: 8, 3: 4}
FACTORS = {2: (2, 4, 8), 3: (2, 4)}


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_decompress_coarse.restype = C.c_int
    lib.dctz_decompress_coarse.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(TVar)]
    lib.dctz_decompress_coarse_box_nd.restype = C.c_int
    lib.dctz_decompress_coarse_box_nd.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(TVar)]
    return lib


def _zvar(z, dtype):
    return _tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])


def _coarse(lib, z, dtype, factor, ext):
    out = np.full(int(np.prod(ext)), np.nan, dtype)
    assert lib.dctz_decompress_coarse(C.byref(_zvar(z, dtype)), factor, C.byref(_tvar(out))) == 1
    return out.reshape(ext)


def _box(lib, z, dtype, factor, lo, hi):
    nd = len(lo)
    m = int(np.prod([max(h - l, 1) for l, h in zip(lo, hi)]))
    out = np.full(m, np.nan, dtype)
    arr = C.c_size_t * nd
    rc = lib.dctz_decompress_coarse_box_nd(C.byref(_zvar(z, dtype)), factor, arr(*lo), arr(*hi), C.byref(_tvar(out)))
    return rc, out


def _boxes(cd, K, seed):
    nd = len(cd)
    bx = [((0,) * nd, tuple(cd)), (tuple(d - 1 for d in cd), tuple(cd)), ((0,) * nd, (1,) * nd)]
    bx.append((tuple(d - max(1, d // 3) for d in cd), tuple(cd)))                       # the far corner: the cells that straddle the edge
    bx.append((tuple(min(K, d - 1) for d in cd), tuple(max(min(K, d - 1) + 1, d - 1) for d in cd)))
    rng = np.random.default_rng(seed)
    for _ in range(6):
        ext = [int(rng.integers(1, d + 1)) for d in cd]
        lo = [int(rng.integers(0, d - x + 1)) for d, x in zip(cd, ext)]
        bx.append((tuple(lo), tuple(l + x for l, x in zip(lo, ext))))
    return bx


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", [(45, 77), (13, 22, 35)], ids=["45x77", "13x22x35"])
def test_coarse_box_is_the_slice_of_the_coarse_container_decode(mode, dtype, shape):
    lib = _lib(mode)
    nd = len(shape)
    x = W.ragged(int(np.prod(shape)), dtype, scale=37.0)
    z, _ = D._container(lib, x, EB, False, shape)
    assert (struct.unpack_from("<I", z, 0)[0] >> 8) & 0xFF == nd
    for f in FACTORS[nd]:
        cd = tuple(-(-d // f) for d in shape)
        whole = _coarse(lib, z, dtype, f, cd)
        for lo, hi in _boxes(cd, EDGE[nd] // f, seed=17 * f + nd):
            rc, r = _box(lib, z, dtype, f, lo, hi)
            assert rc == 1, (f, lo, hi)
            want = np.ascontiguousarray(whole[tuple(slice(l, h) for l, h in zip(lo, hi))])
            assert np.array_equal(r.view(np.uint8), want.reshape(-1).view(np.uint8)), (f, lo, hi)

    def good():
        f = FACTORS[nd][0]
        cd = tuple(-(-d // f) for d in shape)
        rc, r = _box(lib, z, dtype, f, (0,) * nd, cd)
        assert rc == 1 and np.array_equal(r.view(np.uint8), _coarse(lib, z, dtype, f, cd).reshape(-1).view(np.uint8))

    one = ((0,) * nd, (1,) * nd)
    for f in (0, 1, 3, -2, 16, 128) + ((8,) if nd == 3 else ()):                        # a bad factor
        assert _box(lib, z, dtype, f, *one)[0] == -1, f
        good()
    cd = tuple(-(-d // 2) for d in shape)
    outside = [((0,) * nd, tuple(d + 1 if i == a else d for i, d in enumerate(cd))) for a in range(nd)]
    outside += [((0,) * nd, tuple(shape[i] if i == a else d for i, d in enumerate(cd))) for a in range(nd)]   # legal in elements, not in cells
    outside += [(cd, cd), (tuple(d - 1 for d in cd), tuple(d - 1 for d in cd))]         # lo >= hi
    for lo, hi in outside:
        assert _box(lib, z, dtype, 2, lo, hi)[0] == -1, (lo, hi)
        good()
    zf, _ = D._container(lib, x, EB, False, None)                                       # a flat container
    assert (struct.unpack_from("<I", zf, 0)[0] >> 8) & 0xFF == 0
    assert _box(lib, zf, dtype, 2, *one)[0] == -1
    good()
