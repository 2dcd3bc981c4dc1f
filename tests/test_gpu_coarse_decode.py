"""Coarse decode: the whole array at 1 / factor of its resolution from the K = edge / factor low coefficients of every
block (include/dctz_hip.h: dctzhip_decompress_coarse, dctzhip_decompress_coarse_nd).

Reference operator (float64, here): B[i, k] = alpha_N(k) cos(pi k (2i + 1) / (2K)), k < K, applied to the forward orthonormal
DCT of every 64-element block (or tile, separably) of the library's own FULL decode.  Per block
    |coarse - reference| <= 2 K_NOISE eps(T) ||block of the full decode||_2
(tests/noise.py: the yardstick for two correct evaluations of one block transform, doubled because the noise of two
transforms meets: the full decode's and the coarse one's).  At eb >= 1e-3 a one-bin error moves an output by about
2 eb alpha_64 sf = 3.5e-4 sf; the tolerance is at most 2.3e-5 sf (fp32, |x| <= sf): a wrong coefficient cannot hide.

The flat short block (l = n % 64): its ceil(l / factor) values are, bit for bit, the fixed-order means of the cells of the
full decode.  Ragged tiled arrays: bit for bit the leading corner of the coarse decode of the edge-padded array."""
import ctypes as C

import numpy as np
import pytest

from tests.noise import K_NOISE
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

EB = 1e-3
FLAT_N = [37, 4096, 4097, 3 * 4096 + 5 * 64 + 37]
FLAT_F = [2, 4, 8, 16, 32, 64]
ND_F = {2: [2, 4, 8], 3: [2, 4]}
EDGE = {2: 8, 3: 4}
FLAT_CASES = [(n, dt, mode, kind) for n in FLAT_N for dt in (np.float64, np.float32) for mode in (H.EC, H.QT) for kind in ("smooth", "noisy")]
ND_SHAPES = [(24, 40), (72, 80), (8, 12, 16), (20, 20, 20)]
ND_RAGGED = [(21, 35), (7, 9, 10)]
ND_CASES = [(s, dt, mode, kind) for s in ND_SHAPES + ND_RAGGED for dt in (np.float64, np.float32) for mode in (H.EC, H.QT)
            for kind in ("smooth", "noisy")]


def _id(c):
    s, dt, mode, kind = c
    s = "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
    return f"{kind}-{s}-{np.dtype(dt).name}-{'QT' if mode == H.QT else 'EC'}"


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _field(n, kind, dtype, seed):
    """The scaled samples are x / sf with sf the power of ten below max |x| (100 here: 100 < max |x| <= 1000, so the de-scale
    multiply runs); a coefficient beyond 255 eb = 0.255 is stored exactly.  smooth: a scaled block rises by at most 0.014 --
    nothing is stored exactly.  noisy: white noise of scaled sigma = 0.25 on top: about three coefficients in ten are stored
    exactly, at every position (both asserted where they are used)."""
    i = np.arange(n, dtype=np.float64)
    x = 100.0 + 60.0 * np.sin(i / 4000.0) + 6.0 * np.cos(i / 1000.0)
    if kind == "noisy":
        x = x + 25.0 * np.clip(np.random.default_rng(seed).standard_normal(n), -4.0, 4.0)
    return x.astype(dtype)


def _unflagged(b, lo, hi):
    """A position of bin_index[lo, hi) that is not stored exactly and is not a DC slot."""
    for at in range(lo, hi):
        if at % 64 and b[at] != 255:
            return at
    raise AssertionError("every position is stored exactly")


def _alpha(N, k):
    return np.where(k == 0, np.sqrt(1.0 / N), np.sqrt(2.0 / N))


def _fwd(N):
    """F[k, m] = alpha_N(k) cos(pi k (2m + 1) / (2N)): the forward orthonormal DCT (angles reduced in integers)"""
    k = np.arange(N)[:, None]
    m = np.arange(N)[None, :]
    return _alpha(N, k) * np.cos(np.pi * ((k * (2 * m + 1)) % (4 * N)) / (2 * N))


def _basis(N, K):
    """B[i, k] = alpha_N(k) cos(pi k (2i + 1) / (2K)), k < K"""
    i = np.arange(K)[:, None]
    k = np.arange(K)[None, :]
    return _alpha(N, k) * np.cos(np.pi * ((k * (2 * i + 1)) % (4 * K)) / (2 * K))


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


_FLAT = {}


def _flat(ctx, n, dtype, mode, kind):
    """(out, info, full decode (numpy), index, qtable) of one flat workload, compressed and decoded once per module."""
    import torch
    key = (n, np.dtype(dtype).name, mode, kind)
    if key not in _FLAT:
        x = _field(n, kind, dtype, seed=n)
        out, info = ctx.compress(torch.from_numpy(x).to(ctx.device), EB, mode)
        q = np.array(info.qtable[:]) if mode == H.QT else None
        full = ctx.decompress(out, info.cnt, n, _tdt(dtype), EB, info.sf, mode, qtable=q).cpu().numpy()
        idx, tot = ctx.ac_index(out, n)
        assert tot == info.cnt
        _FLAT[key] = (out, info, full, idx, q)
    return _FLAT[key]


def _flags_by_position(out, n):
    """Per in-block position 1 .. 63: how many whole blocks store it exactly."""
    b = out["bin_index"].cpu().numpy()[:n // 64 * 64].reshape(-1, 64)
    f = (b == 255).sum(axis=0)
    f[0] = 0                                            # the DC slot is never an exact coefficient
    return f


def _short_cells(tail, f):
    """The fixed-order means of the cells of the short block: left to right in the data type, divided by the cell's count."""
    dt = tail.dtype.type
    cells = []
    for lo in range(0, tail.size, f):
        hi = min(lo + f, tail.size)
        acc = dt(tail[lo])
        for j in range(lo + 1, hi):
            acc = dt(acc + tail[j])
        cells.append(dt(acc / dt(hi - lo)))
    return np.array(cells, dtype=tail.dtype)


def _check_flat(r, full, n, f, dtype, what):
    K = 64 // f
    nfull = n // 64
    assert r.size == -(-n // f), what
    if nfull:
        blocks = full[:nfull * 64].astype(np.float64).reshape(nfull, 64)
        want = (blocks @ _fwd(64).T)[:, :K] @ _basis(64, K).T
        tol = 2.0 * K_NOISE * float(np.finfo(dtype).eps) * np.sqrt((blocks ** 2).sum(axis=1))
        err = np.abs(r[:nfull * K].astype(np.float64).reshape(nfull, K) - want).max(axis=1)
        print(f"{what}: max err / tol = {float((err / np.maximum(tol, 1e-300)).max()):.3g}")
        assert np.all(err <= tol), (what, float(err.max()), float(tol[np.argmax(err - tol)]))
    if n % 64:
        cells = _short_cells(full[nfull * 64:], f)
        assert np.array_equal(_bits(r[nfull * K:]), _bits(cells)), what


@pytest.mark.parametrize("case", FLAT_CASES, ids=_id)
def test_flat_coarse_is_the_low_band_of_the_full_decode(ctx, case):
    import torch
    n, dtype, mode, kind = case
    out, info, full, idx, q = _flat(ctx, n, dtype, mode, kind)
    tdt = _tdt(dtype)
    if n >= 64:
        fl = _flags_by_position(out, n)
        if kind == "smooth":
            assert fl.sum() == 0
    G = 64                                              # guard elements on each side (keeps d_out 16-byte aligned)
    for f in FLAT_F:
        K = 64 // f
        if kind == "noisy" and n >= 4096 and K >= 2:
            # exact coefficients among the kept positions AND among those passed over: both move a block's place in AC_exact
            assert fl[1:K].sum() > 0 and fl[K:].sum() > 0, (f, fl)
        m = -(-n // f)
        g = torch.empty(m + 2 * G, dtype=tdt, device=ctx.device)
        g.view(torch.int64 if dtype == np.float64 else torch.int32).fill_(0x5A5A5A5A)
        sentinel = g.clone()
        r = ctx.decompress_coarse(out, info.cnt, n, tdt, EB, info.sf, f, index=idx, mode=mode, qtable=q, dst=g[G:G + m])
        tn = "double" if dtype == np.float64 else "float"
        want_k = f"k_decompress_coarse_dc<{tn}>" if K == 1 else f"k_decompress_coarse<{tn}, {mode}, {K}>"
        assert ctx.last_kernel(1) == want_k
        gb, sb = _bits(g.cpu().numpy()), _bits(sentinel.cpu().numpy())
        assert np.array_equal(gb[:G], sb[:G]) and np.array_equal(gb[G + m:], sb[G + m:]), f
        _check_flat(r.cpu().numpy(), full, n, f, dtype, f"{_id(case)} f={f}")
        if f == 64 and n % 64 == 0:
            # the DC stream alone: bin_index, AC_exact and the index passed as NULL
            r2 = ctx.decompress_coarse({"dc": out["dc"]}, 0, n, tdt, EB, info.sf, f, index=None, mode=mode, qtable=q)
            assert np.array_equal(_bits(r2.cpu().numpy()), _bits(r.cpu().numpy()))


def test_coarse_len(ctx):
    for n in (1, 37, 64, 4097):
        for f in FLAT_F:
            assert ctx.lib.dctzhip_coarse_len(n, f) == -(-n // f)
        for f in (0, 1, 3, 48, 128, -2):
            assert ctx.lib.dctzhip_coarse_len(n, f) == 0


# ---- tiled arrays -------------------------------------------------------------------------------------------------------
def _padded_shape(shape):
    e = EDGE[len(shape)]
    return tuple(-(-d // e) * e for d in shape)


_ND = {}


def _nd(ctx, shape, dtype, mode, kind, pad_of=None):
    """(out, info, full decode (numpy), index, qtable) of one tiled workload; the array is _nd_input(shape, ..., pad_of)."""
    import torch
    key = (shape, np.dtype(dtype).name, mode, kind, pad_of)
    if key not in _ND:
        x = _nd_input(shape, dtype, kind, pad_of)
        out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), EB, mode)
        q = np.array(info.qtable[:]) if mode == H.QT else None
        full = ctx.decompress_nd(out, info.cnt, shape, _tdt(dtype), EB, info.sf, mode, qtable=q).cpu().numpy()
        idx, tot = ctx.ac_index(out, 64 * ctx.nd_blocks(shape))
        assert tot == info.cnt
        _ND[key] = (out, info, full, idx, q)
    return _ND[key]


def _nd_input(shape, dtype, kind, pad_of=None):
    """An array of `shape`, or the array of shape `pad_of` edge-padded to `shape`."""
    base = pad_of or shape
    n = int(np.prod(base))
    x = _field(n, kind, dtype, seed=n).reshape(base)
    if base != shape:
        x = np.pad(x, [(0, p - d) for d, p in zip(base, shape)], mode="edge")
    return np.ascontiguousarray(x)


def _nd_reference(full, K, dtype):
    """The operator on every tile of a full decode whose shape is on tile edges -> (coarse array, tolerance per element)."""
    nd = full.ndim
    e = EDGE[nd]
    F, B = _fwd(e), _basis(e, K)
    M = B @ F[:K, :]                                    # element space -> kept coefficients -> coarse values, per axis
    a = full.astype(np.float64)
    nb = [d // e for d in full.shape]
    if nd == 2:
        t = a.reshape(nb[0], e, nb[1], e)
        want = np.einsum("ia,jb,yaxb->yixj", M, M, t).reshape(nb[0] * K, nb[1] * K)
        norm = np.sqrt((t ** 2).sum(axis=(1, 3)))
        tol = np.repeat(np.repeat(norm, K, axis=0), K, axis=1)
    else:
        t = a.reshape(nb[0], e, nb[1], e, nb[2], e)
        want = np.einsum("ia,jb,kc,zaybxc->ziyjxk", M, M, M, t).reshape(nb[0] * K, nb[1] * K, nb[2] * K)
        norm = np.sqrt((t ** 2).sum(axis=(1, 3, 5)))
        tol = np.repeat(np.repeat(np.repeat(norm, K, axis=0), K, axis=1), K, axis=2)
    return want, 2.0 * K_NOISE * float(np.finfo(dtype).eps) * tol


@pytest.mark.parametrize("case", [c for c in ND_CASES if c[0] in ND_SHAPES], ids=_id)
def test_tiled_coarse_is_the_low_band_of_the_full_decode(ctx, case):
    shape, dtype, mode, kind = case
    _check_tiled(ctx, case, _nd(ctx, shape, dtype, mode, kind))


def _check_tiled(ctx, case, data):
    import torch
    shape, dtype, mode, kind = case
    out, info, full, idx, q = data
    tdt = _tdt(dtype)
    nd = len(shape)
    e = EDGE[nd]
    if kind == "noisy":
        b = out["bin_index"].cpu().numpy()[:64 * ctx.nd_blocks(shape)].reshape(-1, 64)
        fl = (b == 255).sum(axis=0)
        fl[0] = 0
    G = 64
    for f in ND_F[nd]:
        K = e // f
        ext = [-(-d // f) for d in shape]
        m = int(np.prod(ext))
        if kind == "noisy" and K >= 2:
            j = np.arange(64)
            kept = ((j // 8 < K) & (j % 8 < K)) if nd == 2 else ((j // 16 < K) & (j // 4 % 4 < K) & (j % 4 < K))
            assert fl[kept].sum() > 0 and fl[~kept & (j < np.flatnonzero(kept)[-1])].sum() > 0 and fl[~kept].sum() > 0, f
        g = torch.empty(m + 2 * G, dtype=tdt, device=ctx.device)
        g.view(torch.int64 if dtype == np.float64 else torch.int32).fill_(0x5A5A5A5A)
        sentinel = g.clone()
        r = ctx.decompress_coarse_nd(out, info.cnt, shape, tdt, EB, info.sf, f, index=idx, mode=mode, qtable=q, dst=g[G:G + m])
        tn = "double" if dtype == np.float64 else "float"
        assert ctx.last_kernel(1) == (f"k_decompress_coarse_dc<{tn}>" if K == 1 else f"k_decompress_coarse_nd<{tn}, {mode}, {nd - 1}, {K}>")
        gb, sb = _bits(g.cpu().numpy()), _bits(sentinel.cpu().numpy())
        assert np.array_equal(gb[:G], sb[:G]) and np.array_equal(gb[G + m:], sb[G + m:]), f
        r = r.cpu().numpy()
        assert list(r.shape) == ext
        want, tol = _nd_reference(full, K, dtype)
        err = np.abs(r.astype(np.float64) - want)
        print(f"{_id(case)} f={f}: max err / tol = {float((err / np.maximum(tol, 1e-300)).max()):.3g}")
        assert np.all(err <= tol), (f, float(err.max()))
        if K == 1:
            r2 = ctx.decompress_coarse_nd({"dc": out["dc"]}, 0, shape, tdt, EB, info.sf, f, index=None, mode=mode, qtable=q)
            assert np.array_equal(_bits(r2.cpu().numpy()), _bits(r))


@pytest.mark.parametrize("case", [c for c in ND_CASES if c[0] in ND_RAGGED], ids=_id)
def test_ragged_coarse_is_the_corner_of_the_padded_one(ctx, case):
    """Edge tiles are padded on compress by repeating the last sample: the streams of the ragged array ARE those of the
    edge-padded one (only the mean differs; sf depends on max |x| alone), and the coarse decode of the ragged array is the
    leading ceil(d / f) corner of the padded one's, which is checked against the operator here."""
    shape, dtype, mode, kind = case
    pshape = _padded_shape(shape)
    out, info, full, idx, q = _nd(ctx, shape, dtype, mode, kind)
    pout, pinfo, pfull, pidx, pq = pdata = _nd(ctx, pshape, dtype, mode, kind, pad_of=shape)
    _check_tiled(ctx, (pshape, dtype, mode, kind), pdata)                       # the padded one against the operator
    assert info.sf == pinfo.sf and info.cnt == pinfo.cnt
    nb = 64 * ctx.nd_blocks(shape)
    assert np.array_equal(out["bin_index"].cpu().numpy()[:nb], pout["bin_index"].cpu().numpy()[:nb])
    assert np.array_equal(out["dc"].cpu().numpy()[:nb // 64].view(np.uint32), pout["dc"].cpu().numpy()[:nb // 64].view(np.uint32))
    assert np.array_equal(out["ac_exact"].cpu().numpy()[:info.cnt].view(np.uint32), pout["ac_exact"].cpu().numpy()[:info.cnt].view(np.uint32))
    tdt = _tdt(dtype)
    for f in ND_F[len(shape)]:
        r = ctx.decompress_coarse_nd(out, info.cnt, shape, tdt, EB, info.sf, f, index=idx, mode=mode, qtable=q).cpu().numpy()
        p = ctx.decompress_coarse_nd(pout, pinfo.cnt, pshape, tdt, EB, pinfo.sf, f, index=pidx, mode=mode, qtable=pq).cpu().numpy()
        ext = [-(-d // f) for d in shape]
        assert list(r.shape) == ext
        corner = np.ascontiguousarray(p[tuple(slice(0, v) for v in ext)])
        assert np.array_equal(_bits(r), _bits(corner)), f


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _raw_flat(ctx, out, cnt, idx_ptr, q, n, tdt, sf, mode, f, dst_ptr, bptr=None, dcptr=None, acptr=None):
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    return ctx.lib.dctzhip_decompress_coarse(ctx.h, out["bin_index"].data_ptr() if bptr is None else bptr,
                                             out["dc"].data_ptr() if dcptr is None else dcptr,
                                             out["ac_exact"].data_ptr() if acptr is None else acptr, int(cnt), idx_ptr, qp, n, H._dt(tdt),
                                             EB, float(sf), mode, f, dst_ptr)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_flat_refusals_leave_the_context_usable(ctx, dtype, mode):
    import torch
    n = FLAT_N[-1]
    out, info, full, idx, q = _flat(ctx, n, dtype, mode, "noisy")
    if q is not None:
        q = np.ascontiguousarray(q, dtype=dtype)
    tdt = _tdt(dtype)
    es = 8 if dtype == np.float64 else 4
    cp = {k: v.clone() for k, v in out.items()}
    dst = torch.empty(n, dtype=tdt, device=ctx.device)
    F = 8
    want = ctx.decompress_coarse(out, info.cnt, n, tdt, EB, info.sf, F, index=idx, mode=mode, qtable=q).cpu().numpy()

    def call(f=F, cnt=info.cnt, ix=idx, ixptr=None, qq=q, dptr=None, o=cp, **kw):
        return _raw_flat(ctx, o, cnt, ix.data_ptr() if ixptr is None else ixptr, qq, n, tdt, info.sf, mode, f,
                         dst.data_ptr() if dptr is None else dptr, **kw)

    def after():
        assert call() == H.OK
        assert np.array_equal(_bits(dst[:want.size].cpu().numpy()), _bits(want))

    after()
    host = [dict(f=v) for v in (0, 1, 3, 48, 128, -2)]
    host += [
        dict(dptr=0), dict(dptr=dst.data_ptr() + es),                           # null / misaligned output
        dict(bptr=0), dict(bptr=cp["bin_index"].data_ptr() + 4),                # ... bin ids
        dict(dcptr=0), dict(dcptr=cp["dc"].data_ptr() + 2),                     # ... DC
        dict(ixptr=0), dict(ixptr=idx.data_ptr() + 2),                          # ... index
        dict(acptr=0), dict(acptr=cp["ac_exact"].data_ptr() + 2),               # null AC_exact with ac_count > 0 / misaligned
        dict(dptr=cp["bin_index"].data_ptr() + 4096),                           # d_out over bin ids
        dict(dptr=cp["dc"].data_ptr()),                                         # ... over DC
        dict(dptr=idx.data_ptr()),                                              # ... over the index
        dict(f=64, bptr=0), dict(f=64, ixptr=0), dict(f=64, acptr=0),           # n % 64 != 0: the short block needs them at factor 64 too
    ]
    if mode == H.QT:
        host.append(dict(qq=None))
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    # one flag added after the index was built: a whole block's position that was not stored exactly, in the second tile
    b = cp["bin_index"].cpu().numpy().copy()
    b[_unflagged(b, 4096 + 64 * 5, 4096 + 64 * 6)] = 255
    bad = dict(cp)
    bad["bin_index"] = torch.from_numpy(b).to(ctx.device)
    for f in (2, 8, 32):
        assert call(o=bad, f=f) == H.E_ARG, f
        after()
    assert call(o=bad, f=64) == H.OK                                            # ... which the DC stream alone does not see (the short block's tile is intact)
    # ... and in the short block (checked by its own kernel, at every factor)
    b = cp["bin_index"].cpu().numpy().copy()
    b[_unflagged(b, n // 64 * 64 + 1, n)] = 255
    bad["bin_index"] = torch.from_numpy(b).to(ctx.device)
    for f in (8, 64):
        assert call(o=bad, f=f) == H.E_ARG, f
        after()
    # an index entry raised by one; ac_count one short
    ix = idx.clone()
    ix[2] += 1
    assert call(ix=ix) == H.E_ARG
    after()
    assert info.cnt > 0
    assert call(cnt=info.cnt - 1) == H.E_ARG
    after()
    for k in out:
        bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert torch.equal(bits(cp[k]), bits(out[k])), k


@pytest.mark.parametrize("shape", [(72, 80), (20, 20, 20)], ids=["72x80", "20x20x20"])
def test_tiled_refusals_leave_the_context_usable(ctx, shape):
    import torch
    dtype, mode = np.float32, H.QT
    out, info, full, idx, q = _nd(ctx, shape, dtype, mode, "noisy")
    q = np.ascontiguousarray(q, dtype=dtype)
    tdt = _tdt(dtype)
    nd = len(shape)
    dst = torch.empty(int(np.prod(shape)), dtype=tdt, device=ctx.device)
    want = ctx.decompress_coarse_nd(out, info.cnt, shape, tdt, EB, info.sf, 2, index=idx, mode=mode, qtable=q).cpu().numpy()

    def call(f=2, dims=shape, ndims=nd, o=out, ixptr=None, qq=q, dptr=None, cnt=info.cnt, bptr=None):
        arr = None if dims is None else (C.c_size_t * len(dims))(*dims)
        return ctx.lib.dctzhip_decompress_coarse_nd(
            ctx.h, o["bin_index"].data_ptr() if bptr is None else bptr, o["dc"].data_ptr(), o["ac_exact"].data_ptr(), int(cnt),
            idx.data_ptr() if ixptr is None else ixptr, qq.ctypes.data_as(C.c_void_p) if qq is not None else None, ndims, arr,
            H._dt(tdt), EB, float(info.sf), mode, f, dst.data_ptr() if dptr is None else dptr)

    def after():
        assert call() == H.OK
        assert np.array_equal(_bits(dst[:want.size].cpu().numpy()), _bits(want.reshape(-1)))

    after()
    host = [dict(f=v) for v in (0, 1, 3, 16, -4) + ((8,) if nd == 3 else ())]
    host += [dict(dims=None), dict(ndims=1, dims=shape[:1]), dict(ndims=4, dims=tuple(shape) + (1,)), dict(dims=(0,) + tuple(shape[1:])),
             dict(dptr=0), dict(dptr=dst.data_ptr() + 4), dict(bptr=0), dict(ixptr=0), dict(ixptr=idx.data_ptr() + 2),
             dict(dptr=out["dc"].data_ptr()), dict(qq=None)]
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    b = out["bin_index"].cpu().numpy().copy()
    b[_unflagged(b, 64 * 70, 64 * 71)] = 255                                    # second stream tile
    bad = dict(out)
    bad["bin_index"] = torch.from_numpy(b).to(ctx.device)
    assert call(o=bad) == H.E_ARG
    after()
    assert call(cnt=info.cnt - 1) == H.E_ARG
    after()


# ---- more tiles than resident workgroups ------------------------------------------------------------------------------------
# k_decompress_coarse and k_decompress_coarse_nd take tiles t, t + gridDim.x, ... and reuse their LDS image between the trips;
# k_decompress_coarse_dc caps its grid at 4096 workgroups and strides.  The arrays are tests/size_cases.py's: a pattern of 257
# (513, 481) stream tiles repeated, then a ragged tail; the model [pattern | tail] is held to the operator above, and the big
# array's coarse decode is, bit for bit, the model's extended period after period.
def _nd_from(ctx, x, mode):
    """_nd's tuple for an array given as such."""
    import torch
    out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), EB, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress_nd(out, info.cnt, x.shape, _tdt(x.dtype.type), EB, info.sf, mode, qtable=q).cpu().numpy()
    idx, tot = ctx.ac_index(out, 64 * ctx.nd_blocks(x.shape))
    assert tot == info.cnt
    return out, info, full, idx, q


@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("kind", ["smooth", "noisy"])
def test_flat_more_tiles_than_resident_workgroups(ctx, kind, mode):
    import torch
    from tests import size_cases as Z
    w, dtype, tdt = Z.C, np.float64, torch.float64
    assert w.tiles > Z.RESIDENT_WAVES
    s = Z.model(w, Z.pattern(w, kind))
    ns = s.size
    sd = torch.from_numpy(s).to(ctx.device)
    outs, infos = ctx.compress(sd, EB, mode)
    q = np.array(infos.qtable[:]) if mode == H.QT else None
    fulls = ctx.decompress(outs, infos.cnt, ns, tdt, EB, infos.sf, mode, qtable=q).cpu().numpy()
    idxs, tot = ctx.ac_index(outs, ns)
    assert tot == infos.cnt and infos.sf == 100.0
    b = Z.expand(sd, w.reps, w.period)
    assert b.numel() == w.n and w.n % 64 == 37
    outb, infob = ctx.compress(b, EB, mode)
    assert infob.sf == infos.sf and bytes(infob.qtable) == bytes(infos.qtable)
    assert Z.streams_ok(w, outb, infob.cnt, outs, infos.cnt)
    idxb, tot = ctx.ac_index(outb, w.n)
    assert tot == infob.cnt
    del b
    fl = _flags_by_position(outs, ns)
    for f in FLAT_F:
        K = 64 // f
        if kind == "noisy" and K >= 2:
            assert fl[1:K].sum() > 0 and fl[K:].sum() > 0, (f, fl)
        rs = ctx.decompress_coarse(outs, infos.cnt, ns, tdt, EB, infos.sf, f, index=idxs, mode=mode, qtable=q)
        _check_flat(rs.cpu().numpy(), fulls, ns, f, dtype, f"model of C {kind} f={f}")
        rb = ctx.decompress_coarse(outb, infob.cnt, w.n, tdt, EB, infob.sf, f, index=idxb, mode=mode, qtable=q)
        assert ctx.last_kernel(1) == ("k_decompress_coarse_dc<double>" if K == 1 else f"k_decompress_coarse<double, {mode}, {K}>")
        assert rb.numel() == -(-w.n // f)
        assert Z.periodic(rb, rs, w.reps, w.period // f), f                     # (the short block's cells are the model's tail)


@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("kind", ["smooth", "noisy"])
@pytest.mark.parametrize("which", ["G2", "G3"])
def test_tiled_more_tiles_than_resident_workgroups(ctx, which, kind, mode):
    """The array-side prefixes of size_cases' G2 (8453 x 8203) and G3 (2307 x 101 x 145), ragged on every axis.  G2's has
    more than 4096 x 256 blocks: at factor 8 k_decompress_coarse_dc strides."""
    import torch
    from tests import size_cases as Z
    w = {"G2": Z.G2_COARSE, "G3": Z.G3_COARSE}[which]
    dtype, tdt, nd = np.float64, torch.float64, len(w.shape)
    assert w.tiles > Z.RESIDENT_WAVES and (which != "G2" or w.stream_n // 64 > Z.DC_GRID_BLOCKS)
    s = Z.model(w, Z.pattern(w, kind))
    shape_s, pshape = s.shape, _padded_shape(s.shape)
    # the model: the padded one against the operator, the ragged one its corner (test_ragged_coarse_is_the_corner_of_the_padded_one)
    outs, infos, fulls, idxs, q = _nd_from(ctx, s, mode)
    pout, pinfo, pfull, pidx, pq = pdata = _nd_from(ctx, np.ascontiguousarray(np.pad(s, [(0, p - d) for d, p in zip(shape_s, pshape)], mode="edge")), mode)
    _check_tiled(ctx, (pshape, dtype, mode, kind), pdata)
    assert infos.sf == pinfo.sf == 100.0 and infos.cnt == pinfo.cnt
    b = Z.expand(torch.from_numpy(s).to(ctx.device), w.reps, w.period)
    assert tuple(b.shape) == w.shape
    outb, infob = ctx.compress_nd(b, EB, mode)
    assert infob.sf == infos.sf and bytes(infob.qtable) == bytes(infos.qtable)
    assert ctx.nd_blocks(w.shape) * 64 == w.stream_n
    assert Z.streams_ok(w, outb, infob.cnt, outs, infos.cnt)
    idxb, tot = ctx.ac_index(outb, w.stream_n)
    assert tot == infob.cnt
    del b
    for f in ND_F[nd]:
        K = EDGE[nd] // f
        rs = ctx.decompress_coarse_nd(outs, infos.cnt, shape_s, tdt, EB, infos.sf, f, index=idxs, mode=mode, qtable=q)
        p = ctx.decompress_coarse_nd(pout, pinfo.cnt, pshape, tdt, EB, pinfo.sf, f, index=pidx, mode=mode, qtable=pq)
        ext = [-(-d // f) for d in shape_s]
        assert list(rs.shape) == ext and Z.same(rs, p[tuple(slice(0, v) for v in ext)].contiguous()), f
        rb = ctx.decompress_coarse_nd(outb, infob.cnt, w.shape, tdt, EB, infob.sf, f, index=idxb, mode=mode, qtable=q)
        assert ctx.last_kernel(1) == ("k_decompress_coarse_dc<double>" if K == 1 else f"k_decompress_coarse_nd<double, {mode}, {nd - 1}, {K}>")
        assert list(rb.shape) == [-(-d // f) for d in w.shape]
        assert Z.periodic(rb, rs, w.reps, w.period // f), f
