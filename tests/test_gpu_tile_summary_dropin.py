"""dctz_tile_summary (include/dctz.h) through the drop-in libraries, EC and QT builds, from a container with the reference's zlib
tail and from one with the DZIX chunk index (DCTZ_ZLIB_GPU=1): records and total are, byte for byte, what the C-ABI call
(dctzhip_tile_summary) gives for the container's inflated streams, with and without the original.  A DZND container, a
reference of the wrong length or type and a call that asks for nothing return -1, and a good call follows."""
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
    lib.dctz_tile_summary.restype = C.c_int
    lib.dctz_tile_summary.argtypes = [C.POINTER(TVar), C.POINTER(TVar), C.c_int, C.c_void_p, C.POINTER(H.TileSummary)]
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


def _summary(lib, z, dtype, ref, n_ref, tiles, want_total=True):
    recs = np.full((max(tiles, 1), 8), np.nan)
    total = H.TileSummary()
    zv = _tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])
    rc = lib.dctz_tile_summary(C.byref(zv), C.byref(_tvar(ref)) if ref is not None else None, n_ref,
                               recs.ctypes.data_as(C.c_void_p) if tiles else None, C.byref(total) if want_total else None)
    return rc, recs[:tiles], total


# a partial last tile plus a short block; whole tiles only
WORK = [(3 * 4096 + 5 * 64 + 37, np.float64), (2 * 4096, np.float32)]


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("work", WORK, ids=lambda w: f"{w[0]}-{np.dtype(w[1]).name}")
@pytest.mark.parametrize("gpu_tail", [False, True], ids=["zlib_tail", "dzix"])
def test_summary_is_the_c_abi_call_on_the_inflated_streams(ctx, mode, work, gpu_tail):
    import torch
    n, dtype = work
    lib = _lib(mode)
    x = W.ragged(n, dtype, scale=37.0)                    # the caller's unscaled original (dctz_compress scales a copy)
    z = _container(lib, x, None, gpu_tail)
    cnt, sf, b, dc, ac, q = _streams(z, dtype, mode == "qt")
    assert b.size == n and ac.size == cnt
    up = lambda a, pad: torch.from_numpy(np.concatenate([a, np.zeros(pad, a.dtype)])).to(ctx.device)
    out = {"bin_index": up(b, 16), "dc": up(dc, 4), "ac_exact": up(ac, 4)}
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    hmode = H.QT if mode == "qt" else H.EC
    tiles = -(-n // 4096)
    xd = torch.from_numpy(x).to(ctx.device)
    for ref, rd in ((None, None), (x, xd)):
        want, wtot = ctx.tile_summary(out, cnt, n, tdt, EB, sf, mode=hmode, qtable=q, ref=rd)
        rc, recs, total = _summary(lib, z, dtype, ref, n, tiles)
        assert rc == 1
        assert np.array_equal(recs.view(np.uint64), want.cpu().numpy().view(np.uint64))
        assert bytes(total) == bytes(wtot)
        rc, _, total = _summary(lib, z, dtype, ref, n, 0)                     # the total alone
        assert rc == 1 and bytes(total) == bytes(wtot)
        rc, recs, _ = _summary(lib, z, dtype, ref, n, tiles, want_total=False)   # the records alone
        assert rc == 1 and np.array_equal(recs.view(np.uint64), want.cpu().numpy().view(np.uint64))
    # refusals: nothing asked for, a reference of the wrong length, of the other type; a good call follows
    assert _summary(lib, z, dtype, x, n, 0, want_total=False)[0] == -1
    assert _summary(lib, z, dtype, x, n - 1, tiles)[0] == -1
    assert _summary(lib, z, dtype, x, n + 64, tiles)[0] == -1
    other = np.float32 if dtype == np.float64 else np.float64
    assert _summary(lib, z, dtype, x.astype(other), n, tiles)[0] == -1
    rc, recs, total = _summary(lib, z, dtype, x, n, tiles)
    assert rc == 1 and bytes(total) == bytes(wtot)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_a_tiled_container_is_refused(ctx, mode):
    lib = _lib(mode)
    shape = (72, 80)
    x = W.ragged(int(np.prod(shape)), np.float64, scale=37.0)
    z = _container(lib, x, shape, False)
    assert _summary(lib, z, np.float64, None, 0, 2)[0] == -1
    assert _summary(lib, z, np.float64, x, x.size, 2)[0] == -1
    zf = _container(lib, x, None, False)                                      # ... and the same array in flat blocks is served
    rc, recs, total = _summary(lib, zf, np.float64, x, x.size, 2)
    assert rc == 1 and total.xmin == float(x.min()) and total.xmax == float(x.max()) and total.emax > 0.0
