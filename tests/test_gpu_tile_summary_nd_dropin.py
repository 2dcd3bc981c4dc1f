"""dctz_tile_summary_nd (include/dctz.h) through the drop-in libraries, EC and QT builds: records and total from a DZND container
are, byte for byte, what Context.tile_summary_nd gives for the container's inflated streams, with and without the original.  A
flat container, a call that asks for nothing, a reference of another type or length and streams that disagree return -1, and
a good call follows."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import ndfix_cases as N
from tests import workloads as W
from tests.dropin_cases import TVar, _tvar
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu
EB = 1e-3
SHAPES = [(72, 80), (13, 22, 35)]     # whole tiles in 2-D (90 blocks: a partial second stream tile); ragged on every axis in 3-D


def _lib(mode):
    lib = D._lib(mode)
    for name in ("dctz_tile_summary_nd", "dctz_tile_summary"):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(TVar), C.POINTER(TVar), C.c_int, C.c_void_p, C.POINTER(H.TileSummary)]
    return lib


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


def _summary(lib, z, dtype, ref, n_ref, tiles, want_total=True, call="dctz_tile_summary_nd"):
    recs = np.full((max(tiles, 1), 8), np.nan)
    total = H.TileSummary()
    zv = _tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])
    rc = getattr(lib, call)(C.byref(zv), C.byref(_tvar(ref)) if ref is not None else None, n_ref,
                            recs.ctypes.data_as(C.c_void_p) if tiles else None, C.byref(total) if want_total else None)
    return rc, recs[:tiles], total


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_summary_is_the_device_call_on_the_inflated_streams(ctx, mode, dtype, shape):
    import torch
    lib = _lib(mode)
    n = int(np.prod(shape))
    x = W.ragged(n, dtype, scale=37.0)                    # the caller's unscaled original (dctz_compress scales a copy)
    z, _ = D._container(lib, x, EB, False, shape)
    cnt, sf, b, dc, ac, q = _streams(z, dtype, mode == "qt")
    n_lin = 64 * N.nblk(shape)
    assert b.size == n_lin and dc.size == N.nblk(shape) and ac.size == cnt
    up = lambda a, pad: torch.from_numpy(np.concatenate([a, np.zeros(pad, a.dtype)])).to(ctx.device)
    out = {"bin_index": up(b, 16), "dc": up(dc, 4), "ac_exact": up(ac, 4)}
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    hmode = H.QT if mode == "qt" else H.EC
    tiles = N.tiles(shape)
    xd = torch.from_numpy(x.reshape(shape)).to(ctx.device)
    for ref, rd in ((None, None), (x, xd)):
        want, wtot = ctx.tile_summary_nd(out, cnt, shape, tdt, EB, sf, mode=hmode, qtable=q, ref=rd)
        rc, recs, total = _summary(lib, z, dtype, ref, n, tiles)
        assert rc == 1
        assert np.array_equal(recs.view(np.uint64), want.cpu().numpy().view(np.uint64))
        assert bytes(total) == bytes(wtot)
        rc, _, total = _summary(lib, z, dtype, ref, n, 0)                     # the total alone
        assert rc == 1 and bytes(total) == bytes(wtot)
        rc, recs, _ = _summary(lib, z, dtype, ref, n, tiles, want_total=False)   # the records alone
        assert rc == 1 and np.array_equal(recs.view(np.uint64), want.cpu().numpy().view(np.uint64))
    assert total is not None and wtot.xmin == float(x.min()) and wtot.xmax == float(x.max()) and wtot.emax > 0.0
    # refusals: nothing asked for; a reference of the wrong length (the stream positions are not the length), of the other type
    assert _summary(lib, z, dtype, x, n, 0, want_total=False)[0] == -1
    assert _summary(lib, z, dtype, x, n - 1, tiles)[0] == -1
    if n_lin != n:
        assert _summary(lib, z, dtype, np.zeros(n_lin, dtype), n_lin, tiles)[0] == -1
    other = np.float32 if dtype == np.float64 else np.float64
    assert _summary(lib, z, dtype, x.astype(other), n, tiles)[0] == -1
    # streams that disagree: the bin ids flag one word more than the header counts
    assert cnt > 0
    bad = z.copy()
    struct.pack_into("<I", bad, 16, cnt - 1)
    rc, recs, total = _summary(lib, bad, dtype, x, n, tiles)
    assert rc == -1 and np.isnan(recs).all() and bytes(total) == bytes(H.TileSummary())
    # the flat call keeps refusing the tiled container, the tiled call refuses a flat one; a good call follows
    assert _summary(lib, z, dtype, x, n, tiles, call="dctz_tile_summary")[0] == -1
    zf, _ = D._container(lib, x, EB, False)
    assert _summary(lib, zf, dtype, x, n, tiles)[0] == -1
    assert _summary(lib, zf, dtype, None, 0, tiles)[0] == -1
    rc, recs, total = _summary(lib, z, dtype, x, n, tiles)
    assert rc == 1 and bytes(total) == bytes(wtot) and np.array_equal(recs.view(np.uint64), want.cpu().numpy().view(np.uint64))
