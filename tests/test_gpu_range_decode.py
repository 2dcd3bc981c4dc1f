"""Random access on decode (include/dctz_hip.h: dctzhip_ac_index, dctzhip_decompress_range).

The exception index against its definition and the oracle's count; the range decode against the slice of a full decode,
bit for bit; locality (everything the contract says is not read is poisoned, the result does not change); output bounds
(a guard around d_out stays untouched); and the refusals, each followed by a good full decode on the same context."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE = 4096
NS = [1, 63, 64, 4095, 4096, 4097, 64 * 777 + 45, (1 << 24) + 29]
# (n, kind): ragged at eb 1e-3 for every n, a dense case (heavy tails at eb 1e-6) and a case with no exceptions at all
WORKLOADS = [(n, "ragged") for n in NS] + [(64 * 777 + 45, "dense"), (TILE * 5 + 17, "none")]
EBS = {"ragged": 1e-3, "dense": 1e-6, "none": 1e-1}


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _input(n, kind, dtype):
    if kind == "ragged":
        return W.ragged(n, dtype, scale=37.0)
    if kind == "dense":
        rng = np.random.default_rng(99)
        base = W.ragged(n, np.float64, scale=37.0) + 200.0 * rng.standard_cauchy(n).clip(-1e3, 1e3)
        return base.astype(dtype)
    return (3.7 * np.sin(np.arange(n) / 97.0)).astype(dtype)


_CACHE = {}


def _case(ctx, n, kind, dtype, mode):
    """(x, out, info, full decode on the device, index, total, eb, qtable) of one workload, compressed once per module."""
    import torch
    key = (n, kind, np.dtype(dtype).name, mode)
    if key not in _CACHE:
        x = _input(n, kind, dtype)
        eb = EBS[kind]
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        out, info = ctx.compress(torch.from_numpy(x).to(ctx.device), eb, mode)
        q = np.array(info.qtable[:]) if mode == H.QT else None
        full = ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, mode, qtable=q)
        idx, tot = ctx.ac_index(out, n)
        _CACHE[key] = (x, out, info, full, idx, tot, eb, q, tdt)
    return _CACHE[key]


def _index_ref(bin_index, n):
    """The definition: flags (bin id 255 at in-block position j >= 1) in elements [0, min(n, 4096 i)), i = 0 .. m."""
    b = np.asarray(bin_index[:n])
    f = (b == 255) & (np.arange(n) % 64 != 0)
    cs = np.concatenate([[0], np.cumsum(f, dtype=np.int64)])
    m = -(-n // TILE)
    return cs[np.minimum(np.arange(m + 1) * TILE, n)]


def _ivw(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_dev(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(_ivw(a), _ivw(b)))


def _ranges(n, seed, k=200):
    nfull = n // 64
    fixed = [(0, n), (0, 1), (n - 1, n), (5, 9), (60, 70), (TILE - 6, TILE + 4), (TILE, 2 * TILE), (2 * TILE - 1, 3 * TILE + 1)]
    if n % 64:
        fixed += [(nfull * 64 + 1, n), (nfull * 64, n), (max(0, nfull * 64 - 3), n)]
    rng = np.random.default_rng(seed + n)
    rnd = []
    for _ in range(k):
        lo = int(rng.integers(0, n))
        ln = int(np.exp(rng.uniform(0.0, np.log(n - lo + 1))))
        rnd.append((lo, min(n, lo + max(1, ln))))
    return [(lo, hi) for lo, hi in fixed + rnd if 0 <= lo < hi <= n]


CASES = [(n, kind, dt, mode) for n, kind in WORKLOADS for dt in (np.float64, np.float32) for mode in (H.EC, H.QT)]


def _id(c):
    n, kind, dt, mode = c
    return f"{kind}-{n}-{np.dtype(dt).name}-{'QT' if mode == H.QT else 'EC'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_index_is_the_prefix_of_the_flags(ctx, case):
    n, kind, dtype, mode = case
    x, out, info, full, idx, tot, eb, q, tdt = _case(ctx, n, kind, dtype, mode)
    m = -(-n // TILE)
    assert idx.numel() == m + 1 == ctx.lib.dctzhip_ac_index_len(n)
    ref = _index_ref(out["bin_index"][:n].cpu().numpy(), n)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ref)
    assert tot == int(idx[m]) == info.cnt
    c = O.compress(x, eb, mode, O.FAST)
    assert c.cnt == tot
    if kind == "none":
        assert tot == 0
    if kind == "dense":
        assert tot > n // 2


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_range_is_the_slice_of_the_full_decode(ctx, case):
    n, kind, dtype, mode = case
    x, out, info, full, idx, tot, eb, q, tdt = _case(ctx, n, kind, dtype, mode)
    for lo, hi in _ranges(n, seed=11):
        r = ctx.decompress_range(out, info.cnt, n, tdt, eb, info.sf, lo, hi, idx, mode, qtable=q)
        assert _same_dev(r, full[lo:hi]), (lo, hi)


def _poisoned(out, idx, n, lo, hi, seed):
    """Copies of the streams and the index with everything outside what [lo, hi) may read overwritten."""
    import torch
    t0, t1 = lo // TILE, -(-hi // TILE)
    rng = np.random.default_rng(seed)
    b = out["bin_index"].clone()
    junk = torch.from_numpy(rng.integers(0, 256, b.numel(), dtype=np.uint8)).to(b.device)
    junk[::7] = 255
    b0, b1 = t0 * TILE, min(n, t1 * TILE)
    keep = b[b0:b1].clone()
    b.copy_(junk)
    b[b0:b1] = keep
    dc = out["dc"].clone()
    keep = dc[t0 * 64:t1 * 64].clone()
    dc.fill_(float("nan"))
    dc[t0 * 64:t1 * 64] = keep
    ac = out["ac_exact"].clone()
    a0, a1 = int(idx[t0]), int(idx[t1])
    keep = ac[a0:a1].clone()
    ac.fill_(float("nan"))
    ac[a0:a1] = keep
    ix = idx.clone()
    keep = ix[t0:t1 + 1].clone()
    ix.fill_(-1)                                     # 0xFFFFFFFF
    ix[t0:t1 + 1] = keep
    return {"bin_index": b, "dc": dc, "ac_exact": ac}, ix


LOCAL = [c for c in CASES if c[0] in (64 * 777 + 45, TILE * 5 + 17, (1 << 24) + 29)]


@pytest.mark.parametrize("case", LOCAL, ids=_id)
def test_range_reads_only_its_tiles(ctx, case):
    n, kind, dtype, mode = case
    x, out, info, full, idx, tot, eb, q, tdt = _case(ctx, n, kind, dtype, mode)
    rng = np.random.default_rng(n)
    rs = [(TILE + 3, 3 * TILE - 5), (TILE * 2, TILE * 3), (n - 70, n), (0, 100), (5 * TILE + 1, 5 * TILE + 2)]
    for _ in range(12):
        lo = int(rng.integers(0, n - 1))
        rs.append((lo, int(min(n, lo + rng.integers(1, 3 * TILE)))))
    for i, (lo, hi) in enumerate(r for r in rs if 0 <= r[0] < r[1] <= n):
        pout, pix = _poisoned(out, idx, n, lo, hi, seed=i)
        r = ctx.decompress_range(pout, info.cnt, n, tdt, eb, info.sf, lo, hi, pix, mode, qtable=q)
        assert _same_dev(r, full[lo:hi]), (lo, hi)


@pytest.mark.parametrize("case", LOCAL, ids=_id)
def test_range_writes_only_its_output(ctx, case):
    import torch
    n, kind, dtype, mode = case
    x, out, info, full, idx, tot, eb, q, tdt = _case(ctx, n, kind, dtype, mode)
    G = 64                                           # guard elements on each side (keeps d_out 16-byte aligned)
    for lo, hi in [(0, 1), (3, 8), (60, 70), (TILE - 1, TILE + 2), (7, 2 * TILE + 3), (n - 1, n), (0, n), (n - 45, n)]:
        if not 0 <= lo < hi <= n:
            continue
        g = torch.empty(hi - lo + 2 * G, dtype=tdt, device=ctx.device)
        _ivw(g).fill_(0x5A5A5A5A)
        sentinel = g.clone()
        dst = g[G:G + hi - lo]
        ctx.decompress_range(out, info.cnt, n, tdt, eb, info.sf, lo, hi, idx, mode, qtable=q, dst=dst)
        assert _same_dev(g[:G], sentinel[:G]) and _same_dev(g[G + hi - lo:], sentinel[G + hi - lo:]), (lo, hi)
        assert _same_dev(dst, full[lo:hi]), (lo, hi)


def _raw(ctx, out, cnt, n, tdt, eb, sf, lo, hi, idx_ptr, mode, q, dst_ptr):
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    return ctx.lib.dctzhip_decompress_range(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                            int(cnt), idx_ptr, qp, n, H._dt(tdt), float(eb), float(sf), mode, lo, hi, dst_ptr)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 64 * 777 + 45 and c[1] == "ragged"], ids=_id)
def test_refusals_leave_the_context_usable(ctx, case):
    import torch
    n, kind, dtype, mode = case
    x, out, info, full, idx, tot, eb, q, tdt = _case(ctx, n, kind, dtype, mode)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    dst = torch.empty(n + 1, dtype=tdt, device=ctx.device)
    # a copy of the streams: a refusal that did not happen must not damage the cached case
    cp = {k: v.clone() for k, v in out.items()}
    es = 8 if dtype == np.float64 else 4

    def after():
        r = ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, mode, qtable=q)
        assert _same_dev(r, full)

    bad = [(5, 5), (6, 5), (0, n + 1)]
    for lo, hi in bad:
        assert _raw(ctx, cp, info.cnt, n, tdt, eb, info.sf, lo, hi, idx.data_ptr(), mode, q, dst.data_ptr()) == H.E_ARG, (lo, hi)
        after()
    # d_out over bin_index (bytes the call reads)
    assert _raw(ctx, cp, info.cnt, n, tdt, eb, info.sf, 0, 100, idx.data_ptr(), mode, q, cp["bin_index"].data_ptr() + 16 * es) == H.E_ARG
    after()
    # one interior index entry raised by 1: the counts of the tiles on both sides of it disagree with their flags
    lo, hi = TILE + 10, 4 * TILE + 10
    t0, t1 = lo // TILE, -(-hi // TILE)
    for t in range(t0 + 1, t1):
        ix = idx.clone()
        ix[t] += 1
        assert _raw(ctx, cp, info.cnt, n, tdt, eb, info.sf, lo, hi, ix.data_ptr(), mode, q, dst.data_ptr()) == H.E_ARG, t
        after()
    # idx[t1] > ac_count
    need = int(idx[t1])
    assert need > 0
    assert _raw(ctx, cp, need - 1, n, tdt, eb, info.sf, lo, hi, idx.data_ptr(), mode, q, dst.data_ptr()) == H.E_ARG
    after()
    # and the range decode itself still works on the same context
    assert _raw(ctx, cp, need, n, tdt, eb, info.sf, lo, hi, idx.data_ptr(), mode, q, dst.data_ptr()) == H.OK
    assert _same_dev(dst[:hi - lo], full[lo:hi])
    for k in out:                                    # bit patterns: AC_exact beyond cnt is uninitialised (NaN != NaN)
        bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert torch.equal(bits(cp[k]), bits(out[k])), k
