"""dctz_decompress_coarse (include/dctz.h) through the drop-in libraries, EC and QT builds, flat and DZND containers, from a
container with the reference's zlib tail and from one with the DZIX chunk index (DCTZ_ZLIB_GPU=1): the result is, byte for
byte, what the C-ABI call (dctzhip_decompress_coarse / dctzhip_decompress_coarse_nd) gives for the container's inflated
streams.  A bad factor returns -1, and a good call follows."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import workloads as W
from tests.dropin_cases import TVar, _tvar
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu
EB = 1e-3


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_decompress_coarse.restype = C.c_int
    lib.dctz_decompress_coarse.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(TVar)]
    return lib


def _container(lib, x, shape, gpu_tail):
    """Container bytes as a uint8 array; shape None: flat blocks."""
    z, _ = D._container(lib, x, EB, gpu_tail, shape)
    assert (struct.unpack_from("<I", z, 0)[0] >> 8) & 0xFF == (len(shape) if shape is not None else 0)
    assert (z[56 + 1] == 0x5E) == bool(gpu_tail)         # the GPU entropy stage's mark
    return z


def _streams(z, dtype, qt):
    """The container's header fields and its three sections inflated with zlib: (cnt, sf, bin_index, DC, AC_exact, qtable)."""
    _, n, eb, cnt = struct.unpack_from("<IIdI", z, 0)
    assert eb == EB
    sf = struct.unpack_from("<d" if dtype == np.float64 else "<f", z, 24)[0]
    sizes = struct.unpack_from("<III", z, 40)
    offs = [56, 56 + sizes[0], 56 + sizes[0] + sizes[1]]
    raw = [zlib.decompress(bytes(z[o:o + s])) for o, s in zip(offs, sizes)]
    q = None
    if qt:
        at = offs[2] + sizes[2]
        q = np.frombuffer(bytes(z[at:at + 64 * np.dtype(dtype).itemsize]), dtype).copy()
    return cnt, sf, np.frombuffer(raw[0], np.uint8), np.frombuffer(raw[1], np.float32), np.frombuffer(raw[2], np.float32), q


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _coarse(lib, z, dtype, factor, m):
    out = np.full(max(m, 1), np.nan, dtype)
    rc = lib.dctz_decompress_coarse(C.byref(_tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])), factor, C.byref(_tvar(out)))
    return rc, out[:m]


# flat: a partial last tile plus a short block, and whole blocks only (factor 64 then inflates the DC section alone)
WORK = [(None, 3 * 4096 + 5 * 64 + 37, np.float64), (None, 2 * 4096, np.float32), ((21, 35), None, np.float32), ((72, 80), None, np.float64),
        ((7, 9, 10), None, np.float64), ((20, 20, 20), None, np.float32)]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=lambda w: ("x".join(map(str, w[0])) if w[0] else str(w[1])) + "-" + np.dtype(w[2]).name)
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_coarse_is_the_c_abi_call_on_the_inflated_streams(ctx, mode, work, gpu_tail):
    import torch
    shape, n, dtype = work
    lib = _lib(mode)
    n = n if shape is None else int(np.prod(shape))
    x = W.ragged(n, dtype, scale=37.0)
    z = _container(lib, x, shape, gpu_tail)
    cnt, sf, b, dc, ac, q = _streams(z, dtype, mode == "qt")
    npos = n if shape is None else 64 * ctx.nd_blocks(shape)
    assert b.size == npos and ac.size == cnt
    up = lambda a, pad: torch.from_numpy(np.concatenate([a, np.zeros(pad, a.dtype)])).to(ctx.device)
    out = {"bin_index": up(b, 16), "dc": up(dc, 4), "ac_exact": up(ac, 4)}
    idx, tot = ctx.ac_index(out, npos)
    assert tot == cnt
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    hmode = H.QT if mode == "qt" else H.EC
    factors = (2, 4, 8, 16, 32, 64) if shape is None else (2, 4, 8) if len(shape) == 2 else (2, 4)
    for f in factors:
        if shape is None:
            want = ctx.decompress_coarse(out, cnt, n, tdt, EB, sf, f, index=idx, mode=hmode, qtable=q).cpu().numpy()
        else:
            want = ctx.decompress_coarse_nd(out, cnt, shape, tdt, EB, sf, f, index=idx, mode=hmode, qtable=q).cpu().numpy()
        rc, r = _coarse(lib, z, dtype, f, want.size)
        assert rc == 1, f
        assert np.array_equal(r.view(np.uint8), want.reshape(-1).view(np.uint8)), f
    # a bad factor returns -1; a good call follows
    for f in (0, 1, 3, -2, 128) + ((16,) if shape is not None else ()) + ((8,) if shape is not None and len(shape) == 3 else ()):
        assert _coarse(lib, z, dtype, f, 1)[0] == -1, f
    rc, r = _coarse(lib, z, dtype, factors[0], want.size * 0 + (-(-n // 2) if shape is None else int(np.prod([-(-d // 2) for d in shape]))))
    assert rc == 1 and np.isfinite(r).all()
