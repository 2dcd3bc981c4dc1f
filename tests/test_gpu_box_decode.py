"""A box of an N-D array in one call (include/dctz_hip.h: dctzhip_decompress_box).

The box against the slice of a full decode, bit for bit; a 1-D box against the range decode; locality (everything outside
the HIT tiles -- those with at least one element in the box -- is poisoned, candidate tiles between hit ones included: the
result does not change); output bounds (a guard around d_out stays untouched); the refusals, each followed by a good
full decode on the same context; and a NaN-poisoned tile that the box straddles.

Shapes: each is the smallest at which one more thing can go wrong (one tile with a short block; whole tiles with rows =
blocks; odd everything; a 2-D row shorter than a tile; 4-D; 1-D; planes of exactly 5 tiles, so that runs of candidate
tiles are not hit; more candidate tiles than resident workgroups)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import nonfinite as NF
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE = 4096
BIG = (160, 256, 256)                                  # 2560 tiles: the grid-stride loop (asserted from the call's own grid)
GAPS = (4, 40, 512)                                    # planes of 5 tiles: boxes leave runs of candidate tiles that are not hit
SHAPES = [(5, 7, 9), (40, 48, 64), (33, 65, 67), (130, 1000), (6, 10, 12, 50), (64 * 777 + 45,), GAPS]
EBS = {"ragged": 1e-3, "dense": 1e-6, "none": 1e-1}
# (shape, kind): ragged at eb 1e-3 for every shape, a dense case (heavy tails at eb 1e-6) and one with no exceptions at all
WORKLOADS = [(s, "ragged") for s in SHAPES] + [((33, 65, 67), "dense"), ((33, 65, 67), "none")]
CASES = [(s, kind, dt, mode) for s, kind in WORKLOADS for dt in (np.float64, np.float32) for mode in (H.EC, H.QT)]
CASES += [(BIG, "ragged", dt, H.EC) for dt in (np.float64, np.float32)]


def _id(c):
    s, kind, dt, mode = c
    return f"{kind}-{'x'.join(map(str, s))}-{np.dtype(dt).name}-{'QT' if mode == H.QT else 'EC'}"


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


def _case(ctx, shape, kind, dtype, mode):
    """(out, info, full decode on the device, index, eb, qtable, torch dtype) of one workload, compressed once per module."""
    import torch
    n = int(np.prod(shape))
    key = (n, kind, np.dtype(dtype).name, mode)
    if key not in _CACHE:
        x = _input(n, kind, dtype)
        eb = EBS[kind]
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        out, info = ctx.compress(torch.from_numpy(x).to(ctx.device), eb, mode)
        q = np.array(info.qtable[:]) if mode == H.QT else None
        full = ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, mode, qtable=q)
        idx, tot = ctx.ac_index(out, n)
        assert tot == info.cnt
        _CACHE[key] = (out, info, full, idx, eb, q, tdt)
    return _CACHE[key]


def _ivw(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_dev(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(_ivw(a.contiguous()), _ivw(b.contiguous())))


def _slice(full, shape, lo, hi):
    return full.view(shape)[tuple(slice(l, h) for l, h in zip(lo, hi))].contiguous()


def _corners(shape):
    return [(tuple(c), tuple(v + 1 for v in c)) for c in itertools.product(*[sorted({0, d - 1}) for d in shape])]


def _odd_box(shape):
    """Fastest start and extent odd (fp64 output chunks misaligned in every other row), the other dimensions cut on both sides."""
    lo = [d // 4 for d in shape]
    hi = [max(l + 1, d - d // 4) for l, d in zip(lo, shape)]
    d = shape[-1]
    lo[-1] = min(1, d - 1)
    ext = max(1, min(d - lo[-1], 2 * (d // 3) + 1))
    ext -= 1 - ext % 2 if ext > 1 else 0
    hi[-1] = lo[-1] + ext
    return tuple(lo), tuple(hi)


def _boxes(shape, seed, k=40):
    nd, n = len(shape), int(np.prod(shape))
    short, full_end = n % 64, n // 64 * 64
    bx = [((0,) * nd, tuple(shape))] + _corners(shape)
    mid = tuple(d // 2 for d in shape[:-1])
    bx.append((mid + (0,), tuple(v + 1 for v in mid) + (shape[-1],)))                 # one full row
    for a in range(nd):                                                               # a one-thick slab along every axis
        at = shape[a] // 3
        bx.append((tuple(at if i == a else 0 for i in range(nd)), tuple(at + 1 if i == a else shape[i] for i in range(nd))))
    bx.append(_odd_box(shape))
    bx.append((tuple(d - max(1, d // 3) for d in shape), tuple(shape)))               # ends at the array's last element
    if short:
        last = tuple(d - 1 for d in shape[:-1])
        kk = min(short, shape[-1])                                                    # only elements of the short block
        bx.append((last + (shape[-1] - kk,), tuple(shape)))
        c = np.unravel_index(full_end - 1, shape)                                     # ends one element before the short block
        bx.append((tuple(int(v) for v in c[:-1]) + (max(0, int(c[-1]) - 5),), tuple(int(v) + 1 for v in c)))
    rng = np.random.default_rng(seed + n)
    for _ in range(k):                                                                # log-uniform extents
        ext = [max(1, min(d, int(np.exp(rng.uniform(0.0, np.log(d + 1)))))) for d in shape]
        lo = [int(rng.integers(0, d - e + 1)) for d, e in zip(shape, ext)]
        bx.append((tuple(lo), tuple(l + e for l, e in zip(lo, ext))))
    for lo, hi in bx:
        assert all(0 <= l < h <= d for l, h, d in zip(lo, hi, shape)), (lo, hi)
    return bx


def _box(ctx, case_data, shape, lo, hi, mode, out=None, idx=None, cnt=None, dst=None):
    o, info, full, ix, eb, q, tdt = case_data
    return ctx.decompress_box(out or o, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, lo, hi, ix if idx is None else idx,
                              mode, qtable=q, dst=dst)


def test_short_block_boxes_are_what_they_claim():
    """(no GPU work) the two boxes built around the short block lie where their names say."""
    for shape in SHAPES:
        n = int(np.prod(shape))
        if n % 64 == 0:
            continue
        flat = np.arange(n).reshape(shape)
        only, before = _boxes(shape, 0, k=0)[-2:]
        sel = flat[tuple(slice(l, h) for l, h in zip(*only))]
        assert sel.min() >= n // 64 * 64
        sel = flat[tuple(slice(l, h) for l, h in zip(*before))]
        assert sel.max() == n // 64 * 64 - 1


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_box_is_the_slice_of_the_full_decode(ctx, case):
    shape, kind, dtype, mode = case
    data = _case(ctx, shape, kind, dtype, mode)
    full = data[2]
    for lo, hi in _boxes(shape, seed=5):
        r = _box(ctx, data, shape, lo, hi, mode)
        assert tuple(r.shape) == tuple(h - l for l, h in zip(lo, hi))
        assert _same_dev(r, _slice(full, shape, lo, hi)), (lo, hi)
    if shape == BIG:                                   # the whole array: more candidate tiles than workgroups launched
        _box(ctx, data, shape, (0, 0, 0), shape, mode)
        assert ctx.counter(12) == int(np.prod(shape)) // TILE and ctx.counter(11) < ctx.counter(12)
    assert ctx.last_kernel(1) == f"k_decompress_box<{'double' if dtype == np.float64 else 'float'}, {mode}>"


@pytest.mark.parametrize("case", [c for c in CASES if len(c[0]) == 1], ids=_id)
def test_box_of_one_dimension_is_the_range_decode(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = _case(ctx, shape, kind, dtype, mode)
    n = shape[0]
    for lo, hi in _boxes(shape, seed=7):
        r = _box(ctx, data, shape, lo, hi, mode)
        ref = ctx.decompress_range(out, info.cnt, n, tdt, eb, info.sf, lo[0], hi[0], idx, mode, qtable=q)
        assert _same_dev(r, ref), (lo, hi)


def _hit_tiles(shape, lo, hi):
    """From a boolean mask of the box over the flat array: (hit per tile, t0, t1)."""
    n = int(np.prod(shape))
    m = np.zeros(shape, bool)
    m[tuple(slice(l, h) for l, h in zip(lo, hi))] = True
    flat = np.zeros(-(-n // TILE) * TILE, bool)
    flat[:n] = m.reshape(-1)
    hit = flat.reshape(-1, TILE).any(axis=1)
    t = np.flatnonzero(hit)
    return hit, int(t[0]), int(t[-1]) + 1


def _poisoned(out, idx, n, hit, seed):
    """Copies of the streams and the index with everything the contract excludes overwritten."""
    import torch
    dev = idx.device
    rng = np.random.default_rng(seed)
    nblk = -(-n // 64)
    b = out["bin_index"].cpu().numpy().copy()
    junk = rng.integers(0, 256, b.size, dtype=np.uint8)
    junk[::7] = 255
    eh = np.zeros(b.size, bool)
    eh[:n] = np.repeat(hit, TILE)[:n]
    b = np.where(eh, b, junk)
    dc = out["dc"].cpu().numpy().copy()
    bh = np.zeros(dc.size, bool)
    bh[:nblk] = np.repeat(hit, 64)[:nblk]
    dc[~bh] = np.nan
    ix = idx.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    ac = out["ac_exact"].cpu().numpy().copy()
    keep = np.zeros(ac.size, bool)
    for t in np.flatnonzero(hit):
        keep[ix[t]:ix[t + 1]] = True
    ac[~keep] = np.nan
    used = np.zeros(ix.size, bool)
    used[:-1] |= hit
    used[1:] |= hit
    pix = np.where(used, ix, 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {"bin_index": up(b), "dc": up(dc), "ac_exact": up(ac)}, up(pix)


# boxes whose candidate span contains non-hit tiles between hit ones (asserted below from the mask)
# ((33, 65, 67) has planes of 4355 elements: a tile of 4096 escapes a box only where a thin box leaves it whole, so
# [2:30, 10:20, 5:9] hits every candidate tile and [2:30, 10:11, 5:9] is used instead)
LOCAL_BOXES = {
    (33, 65, 67): [((2, 10, 5), (30, 11, 9)), ((0, 64, 60), (33, 65, 67))],
    (6, 10, 12, 50): [((1, 2, 0, 10), (5, 4, 12, 20)), ((0, 0, 3, 7), (6, 1, 4, 8))],
    GAPS: [((1, 3, 100), (3, 5, 200)), ((0, 39, 0), (4, 40, 512)), ((0, 0, 5), (4, 1, 6))],
    BIG: [((10, 100, 30), (20, 110, 200))],
}
LOCAL = [c for c in CASES if c[0] in LOCAL_BOXES and c[1] == "ragged"] + [c for c in CASES if c[1] == "dense"]


@pytest.mark.parametrize("case", LOCAL, ids=_id)
def test_box_reads_only_the_tiles_it_hits(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = _case(ctx, shape, kind, dtype, mode)
    n = int(np.prod(shape))
    gaps = 0
    for i, (lo, hi) in enumerate(LOCAL_BOXES[shape]):
        hit, t0, t1 = _hit_tiles(shape, lo, hi)
        gaps += int((~hit[t0:t1]).sum())
        pout, pix = _poisoned(out, idx, n, hit, seed=i)
        r = _box(ctx, data, shape, lo, hi, mode, out=pout, idx=pix)
        assert _same_dev(r, _slice(full, shape, lo, hi)), (lo, hi)
    assert gaps > 0, "no box of this shape leaves a candidate tile that is not hit"
    if shape in (GAPS, BIG):                           # every box of these: runs of non-hit tiles inside [t0, t1)
        for lo, hi in LOCAL_BOXES[shape]:
            hit, t0, t1 = _hit_tiles(shape, lo, hi)
            assert (~hit[t0:t1]).sum() >= 2, (lo, hi)


GUARDED = [c for c in CASES if c[0] in ((5, 7, 9), (33, 65, 67), (130, 1000)) and c[1] == "ragged"]


@pytest.mark.parametrize("case", GUARDED, ids=_id)
def test_box_writes_only_its_output(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    data = _case(ctx, shape, kind, dtype, mode)
    full, tdt = data[2], data[6]
    G = 64                                             # guard elements on each side (keeps d_out 16-byte aligned)
    for lo, hi in _corners(shape) + [_odd_box(shape), ((0,) * len(shape), tuple(shape))]:
        cnt = int(np.prod([h - l for l, h in zip(lo, hi)]))
        g = torch.empty(cnt + 2 * G, dtype=tdt, device=ctx.device)
        _ivw(g).fill_(0x5A5A5A5A)
        sentinel = g.clone()
        r = _box(ctx, data, shape, lo, hi, mode, dst=g[G:G + cnt])
        assert _same_dev(g[:G], sentinel[:G]) and _same_dev(g[G + cnt:], sentinel[G + cnt:]), (lo, hi)
        assert _same_dev(r, _slice(full, shape, lo, hi)), (lo, hi)


def _raw(ctx, out, cnt, n, tdt, eb, sf, nd, dims, lo, hi, idx_ptr, mode, q, dst_ptr):
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = lambda v: None if v is None else (C.c_size_t * len(v))(*v)
    return ctx.lib.dctzhip_decompress_box(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                          int(cnt), idx_ptr, qp, n, H._dt(tdt), float(eb), float(sf), mode, nd, arr(dims), arr(lo),
                                          arr(hi), dst_ptr)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == GAPS], ids=_id)
def test_refusals_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = _case(ctx, shape, kind, dtype, mode)
    n = int(np.prod(shape))
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    dst = torch.empty(n + 2, dtype=tdt, device=ctx.device)
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    es = 8 if dtype == np.float64 else 4
    D, L, Hh = list(shape), [1, 3, 100], [3, 5, 200]

    def call(nd=3, dims=D, lo=L, hi=Hh, ix=idx, cnt=info.cnt, dptr=None, nn=n):
        return _raw(ctx, cp, cnt, nn, tdt, eb, info.sf, nd, dims, lo, hi, ix.data_ptr(), mode, q, dst.data_ptr() if dptr is None else dptr)

    def after():
        r = ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, mode, qtable=q)
        assert _same_dev(r, full)

    big = 1 << 62
    host = [
        dict(nd=0), dict(nd=5, dims=D + [1, 1], lo=L + [0, 0], hi=Hh + [1, 1]), dict(nd=-1),
        dict(dims=None), dict(lo=None), dict(hi=None),
        dict(dims=[4, 0, 512]),                                                 # a zero extent of the array
        dict(lo=[1, 3, 100], hi=[3, 3, 200]),                                   # ... of the box
        dict(lo=[1, 4, 100], hi=[3, 3, 200]),
        dict(hi=[3, 5, 513]), dict(hi=[5, 5, 200]),
        dict(dims=[4, 40, 511]), dict(dims=[4, 41, 512]),                       # prod dims != n
        dict(dims=[big, 8, big], lo=[0, 0, 0], hi=[1, 1, 1]),                   # ... a product that wraps around to n's size
        dict(dims=[big, 4, n], lo=[0, 0, 0], hi=[1, 1, 1]),
        dict(dptr=0), dict(dptr=dst.data_ptr() + es),                           # null / misaligned output
        dict(dptr=cp["bin_index"].data_ptr() + (1 * 40 * 512 + 3 * 512) // 16 * 16),   # d_out over bin ids the call reads
    ]
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    hit, t0, t1 = _hit_tiles(shape, L, Hh)
    th = np.flatnonzero(hit)
    # an index entry raised by 1 at a hit tile (its own entry, and the one behind it)
    for t in (int(th[0]), int(th[0]) + 1, int(th[-1])):
        ix = idx.clone()
        ix[t] += 1
        assert call(ix=ix) == H.E_ARG, t
        after()
    # the same at entries that belong to no hit tile, inside the candidate span: not read
    free = [t for t in range(t0 + 1, t1) if not hit[t] and not hit[t - 1]]
    assert free
    for t in free[:3]:
        ix = idx.clone()
        ix[t] += 1
        assert call(ix=ix) == H.OK, t
        assert _same_dev(dst[:2 * 2 * 100].view(2, 2, 100), _slice(full, shape, L, Hh))
    # ac_count one short of what the last hit tile needs
    need = int(idx[int(th[-1]) + 1])
    assert need > 0
    assert call(cnt=need - 1) == H.E_ARG
    after()
    assert call(cnt=need) == H.OK
    assert _same_dev(dst[:2 * 2 * 100].view(2, 2, 100), _slice(full, shape, L, Hh))
    for k in out:                                      # bit patterns: AC_exact beyond cnt is uninitialised (NaN != NaN)
        bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert torch.equal(bits(cp[k]), bits(out[k])), k


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_box_over_a_nan_tile_is_the_slice(ctx, dtype, mode):
    """tests/nonfinite.py's poisoned tile (every block of one interior tile holds a NaN): a box that starts before it and
    ends behind it equals the slice of the full decode under that module's rule."""
    import torch
    shape = (33, 65, 67)
    n = int(np.prod(shape))
    x, bad = NF.make("nan_tile", n, dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out, info = ctx.compress(torch.from_numpy(x).to(ctx.device), 1e-3, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress(out, info.cnt, n, tdt, 1e-3, info.sf, mode, qtable=q)
    idx, _ = ctx.ac_index(out, n)
    first, last = np.unravel_index(int(bad[0]) * 64, shape), np.unravel_index(min(int(bad[-1]) * 64 + 63, n - 1), shape)
    lo, hi = (int(first[0]) - 2, 3, 1), (int(last[0]) + 3, 60, 66)
    assert 0 <= lo[0] and hi[0] <= shape[0]
    want = _slice(full, shape, lo, hi).cpu().numpy()
    assert np.isnan(want).any() and not np.isnan(want).all()
    r = ctx.decompress_box(out, info.cnt, shape, tdt, 1e-3, info.sf, lo, hi, idx, mode, qtable=q).cpu().numpy()
    assert NF.same_with_nans(r, want), NF.describe_mismatch(r, want)
