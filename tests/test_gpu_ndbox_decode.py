"""A box of an array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one call (include/dctz_hip.h: dctzhip_decompress_box_nd).

The box against the slice of the full dctzhip_decompress_nd, bit for bit, and against the CPU oracle's decompress_nd;
locality (everything outside the HIT stream tiles -- 64 consecutive blocks with at least one block that intersects the box
-- is poisoned, candidate tiles between hit ones included: the result does not change); output bounds (a guard around
d_out stays untouched); a NaN block that the box straddles; the refusals, each followed by a good call on the same
context.

Shapes: each is the smallest at which one more thing can go wrong (one block; ragged on both axes under one tile; a tile
that spans two block rows and a two-block last tile; unpadded with a tile = one block row, where the full decode writes
the array in place; the same in 3-D; runs of candidate tiles that are not hit; more candidate tiles than resident
workgroups)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import nonfinite as NF
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE_BLKS = 64
EDGE = {2: 8, 3: 4}
BIG = (256, 256, 160)                                  # 2560 tiles: the grid-stride loop (asserted from the call's own grid)
GAPS = (12, 64, 256)                                   # a tile = one (z, y) block row: a box thin in y leaves candidate tiles that are not hit
RAGGED3 = (13, 22, 35)
SHAPES = [(8, 8), (45, 77), (16, 520), (64, 512), (4, 4, 4), RAGGED3, (16, 16, 32), GAPS]
EBS = {"ragged": 1e-3, "dense": 1e-6, "none": 1e-1}
WORKLOADS = [(s, "ragged") for s in SHAPES] + [(RAGGED3, "dense"), (RAGGED3, "none")]
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


def _input(shape, kind, dtype):
    n = int(np.prod(shape))
    if kind == "ragged":
        x = W.ragged(n, dtype, scale=37.0)
    elif kind == "dense":
        rng = np.random.default_rng(99)
        x = (W.ragged(n, np.float64, scale=37.0) + 200.0 * rng.standard_cauchy(n).clip(-1e3, 1e3)).astype(dtype)
    else:
        x = (3.7 * np.sin(np.arange(n) / 97.0)).astype(dtype)
    return np.ascontiguousarray(x.reshape(shape))


def _nblk(shape):
    e = EDGE[len(shape)]
    return int(np.prod([-(-d // e) for d in shape]))


_CACHE = {}


def _case(ctx, shape, kind, dtype, mode):
    """(out, info, full decode on the device, index, eb, qtable, torch dtype) of one workload, compressed once per module."""
    import torch
    key = (shape, kind, np.dtype(dtype).name, mode)
    if key not in _CACHE:
        x = _input(shape, kind, dtype)
        eb = EBS[kind]
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), eb, mode)
        q = np.array(info.qtable[:]) if mode == H.QT else None
        full = ctx.decompress_nd(out, info.cnt, shape, tdt, eb, info.sf, mode, qtable=q)
        idx, tot = ctx.ac_index(out, 64 * _nblk(shape))
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


def _clamped(shape, lo, hi):
    lo = [min(max(l, 0), d - 1) for l, d in zip(lo, shape)]
    hi = [min(max(h, l + 1), d) for l, h, d in zip(lo, hi, shape)]
    return tuple(lo), tuple(hi)


def _aligned(shape):
    """A box on block edges on all sides (clamped to the array where it is ragged)."""
    e = EDGE[len(shape)]
    nb = [-(-d // e) for d in shape]
    lo = [e * (b // 4) for b in nb]
    hi = [e * max(b // 4 + 1, b - b // 4) for b in nb]
    return _clamped(shape, lo, hi)


def _odd_box(shape):
    """Fastest start and extent odd, the other dimensions cut on both sides."""
    lo = [d // 4 for d in shape]
    hi = [max(l + 1, d - d // 4) for l, d in zip(lo, shape)]
    d = shape[-1]
    lo[-1] = min(1, d - 1)
    ext = max(1, min(d - lo[-1], 2 * (d // 3) + 1))
    ext -= 1 - ext % 2 if ext > 1 else 0
    hi[-1] = lo[-1] + ext
    return tuple(lo), tuple(hi)


def _boxes(shape, seed, k=40):
    nd = len(shape)
    e = EDGE[nd]
    bx = [((0,) * nd, tuple(shape))] + _corners(shape)
    for a in range(nd):                                                               # a one-thick slab along every axis
        at = shape[a] // 3
        bx.append((tuple(at if i == a else 0 for i in range(nd)), tuple(at + 1 if i == a else shape[i] for i in range(nd))))
    alo, ahi = _aligned(shape)
    bx.append((alo, ahi))
    bx.append(_clamped(shape, [l + 1 for l in alo], [h + 1 for h in ahi]))            # the same box moved by +1 ...
    bx.append(_clamped(shape, [l - 1 for l in alo], [h - 1 for h in ahi]))            # ... and by -1 on every side
    bx.append(_clamped(shape, [l + 1 for l in alo], [h - 1 for h in ahi]))
    bx.append(_clamped(shape, [l - 1 for l in alo], [h + 1 for h in ahi]))
    org = [e * ((d - 1) // e // 2) for d in shape]                                    # inside a single block
    bx.append(_clamped(shape, [o + 1 for o in org], [o + e - 1 for o in org]))
    bx.append((tuple(d - max(1, d // 3) for d in shape), tuple(shape)))               # ends at the array's last element
    bx.append(_odd_box(shape))
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    for _ in range(k):                                                                # log-uniform extents
        ext = [max(1, min(d, int(np.exp(rng.uniform(0.0, np.log(d + 1)))))) for d in shape]
        lo = [int(rng.integers(0, d - x + 1)) for d, x in zip(shape, ext)]
        bx.append((tuple(lo), tuple(l + x for l, x in zip(lo, ext))))
    for lo, hi in bx:
        assert all(0 <= l < h <= d for l, h, d in zip(lo, hi, shape)), (lo, hi)
    return bx


def test_boxes_are_what_they_claim():
    """(no GPU work) the aligned box lies on block edges, the single-block box inside one block, the odd box is odd."""
    for shape in SHAPES + [BIG]:
        e = EDGE[len(shape)]
        lo, hi = _aligned(shape)
        assert all(l % e == 0 and (h % e == 0 or h == d) for l, h, d in zip(lo, hi, shape))
        bx = _boxes(shape, 0, k=0)
        lo, hi = bx[-3]
        assert all(l // e == (h - 1) // e for l, h in zip(lo, hi))
        lo, hi = bx[-1]
        assert shape[-1] < 3 or (lo[-1] % 2 == 1 and (hi[-1] - lo[-1]) % 2 == 1)
        assert bx[-2][1] == tuple(shape)


def _box(ctx, case_data, shape, lo, hi, mode, out=None, idx=None, cnt=None, dst=None):
    o, info, full, ix, eb, q, tdt = case_data
    return ctx.decompress_box_nd(out or o, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, lo, hi, ix if idx is None else idx,
                                 mode, qtable=q, dst=dst)


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
        assert ctx.counter(12) == _nblk(shape) // TILE_BLKS == 2560 and ctx.counter(11) < ctx.counter(12)
    assert ctx.last_kernel(1) == f"k_decompress_ndbox<{'double' if dtype == np.float64 else 'float'}, {mode}, {len(shape) - 1}>"


ORACLE = [((45, 77), np.float64, H.EC), ((45, 77), np.float32, H.QT), (RAGGED3, np.float64, H.QT), (RAGGED3, np.float32, H.EC)]


@pytest.mark.parametrize("case", ORACLE, ids=lambda c: _id((c[0], "ragged", c[1], c[2])))
def test_box_is_the_slice_of_the_oracle(ctx, case):
    import oracle.oracle as O
    shape, dtype, mode = case
    data = _case(ctx, shape, "ragged", dtype, mode)
    x = _input(shape, "ragged", dtype)
    ref = O.decompress_nd(O.compress_nd(x, EBS["ragged"], O.QT if mode == H.QT else O.EC), shape)
    u = np.uint64 if dtype == np.float64 else np.uint32
    for lo, hi in _boxes(shape, seed=11, k=10):
        r = _box(ctx, data, shape, lo, hi, mode).cpu().numpy()
        want = np.ascontiguousarray(ref[tuple(slice(l, h) for l, h in zip(lo, hi))])
        assert r.shape == want.shape and np.array_equal(r.view(u), want.view(u)), (lo, hi)


def _hit_tiles(shape, lo, hi):
    """From the contract: the blocks [lo / e, (hi - 1) / e] per axis, a mask over the row-major block grid, 64 blocks to a
    stream tile -> (hit per tile, t0, t1)."""
    e = EDGE[len(shape)]
    nb = [-(-d // e) for d in shape]
    m = np.zeros(nb, bool)
    m[tuple(slice(l // e, (h - 1) // e + 1) for l, h in zip(lo, hi))] = True
    nblk = int(np.prod(nb))
    flat = np.zeros(-(-nblk // TILE_BLKS) * TILE_BLKS, bool)
    flat[:nblk] = m.reshape(-1)
    hit = flat.reshape(-1, TILE_BLKS).any(axis=1)
    t = np.flatnonzero(hit)
    return hit, int(t[0]), int(t[-1]) + 1


def _poisoned(out, idx, nblk, hit, seed):
    """Copies of the streams and the index with everything the contract excludes overwritten."""
    import torch
    dev = idx.device
    rng = np.random.default_rng(seed)
    n = 64 * nblk
    b = out["bin_index"].cpu().numpy().copy()
    junk = rng.integers(0, 256, b.size, dtype=np.uint8)
    junk[::7] = 255
    eh = np.zeros(b.size, bool)
    eh[:n] = np.repeat(hit, 64 * TILE_BLKS)[:n]
    b = np.where(eh, b, junk)
    dc = out["dc"].cpu().numpy().copy()
    bh = np.zeros(dc.size, bool)
    bh[:nblk] = np.repeat(hit, TILE_BLKS)[:nblk]
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


# (the boxes of GAPS and BIG leave runs of candidate tiles that are not hit: asserted below from the mask)
LOCAL_BOXES = {
    (16, 520): [((0, 0), (8, 8)), ((9, 500), (16, 520)), ((3, 100), (4, 101))],
    (64, 512): [((8, 0), (16, 512)), ((17, 3), (40, 5)), ((63, 511), (64, 512))],
    RAGGED3: [((0, 0, 0), (4, 8, 35)), ((12, 21, 34), (13, 22, 35)), ((5, 9, 3), (7, 11, 30))],
    (16, 16, 32): [((0, 0, 0), (1, 1, 1)), ((8, 0, 0), (16, 16, 32)), ((7, 15, 31), (9, 16, 32))],
    GAPS: [((0, 20, 10), (12, 22, 200)), ((1, 63, 0), (9, 64, 256)), ((0, 0, 5), (12, 1, 6))],
    BIG: [((10, 100, 30), (20, 110, 150))],
}
LOCAL = [c for c in CASES if c[0] in LOCAL_BOXES and c[1] == "ragged"] + [c for c in CASES if c[1] == "dense"]


@pytest.mark.parametrize("case", LOCAL, ids=_id)
def test_box_reads_only_the_tiles_it_hits(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = _case(ctx, shape, kind, dtype, mode)
    gaps = 0
    for i, (lo, hi) in enumerate(LOCAL_BOXES[shape]):
        hit, t0, t1 = _hit_tiles(shape, lo, hi)
        gaps += int((~hit[t0:t1]).sum())
        pout, pix = _poisoned(out, idx, _nblk(shape), hit, seed=i)
        r = _box(ctx, data, shape, lo, hi, mode, out=pout, idx=pix)
        assert _same_dev(r, _slice(full, shape, lo, hi)), (lo, hi)
    if shape in (GAPS, BIG):                           # every box of these: runs of non-hit tiles inside [t0, t1)
        assert gaps > 0
        for lo, hi in LOCAL_BOXES[shape]:
            hit, t0, t1 = _hit_tiles(shape, lo, hi)
            assert (~hit[t0:t1]).sum() >= 2, (lo, hi)


GUARDED = [c for c in CASES if c[0] in ((8, 8), (45, 77), (64, 512), RAGGED3, (16, 16, 32)) and c[1] == "ragged"]


@pytest.mark.parametrize("case", GUARDED, ids=_id)
def test_box_writes_only_its_output(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    data = _case(ctx, shape, kind, dtype, mode)
    full, tdt = data[2], data[6]
    G = 64                                             # guard elements on each side (keeps d_out 16-byte aligned)
    for lo, hi in _corners(shape) + [_odd_box(shape), _aligned(shape), ((0,) * len(shape), tuple(shape))]:
        cnt = int(np.prod([h - l for l, h in zip(lo, hi)]))
        g = torch.empty(cnt + 2 * G, dtype=tdt, device=ctx.device)
        _ivw(g).fill_(0x5A5A5A5A)
        sentinel = g.clone()
        r = _box(ctx, data, shape, lo, hi, mode, dst=g[G:G + cnt])
        assert _same_dev(g[:G], sentinel[:G]) and _same_dev(g[G + cnt:], sentinel[G + cnt:]), (lo, hi)
        assert _same_dev(r, _slice(full, shape, lo, hi)), (lo, hi)


@pytest.mark.parametrize("shape", [(45, 77), RAGGED3], ids=["45x77", "13x22x35"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_box_over_a_nan_block_is_the_slice(ctx, shape, dtype, mode):
    """A NaN in one block: a box that straddles the block is NaN exactly where the full decode is NaN, and keeps the same
    bits everywhere else (tests/nonfinite.py's rule)."""
    import torch
    x = _input(shape, "ragged", dtype)
    at = tuple(d // 2 for d in shape)
    x[at] = np.nan
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), 1e-3, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress_nd(out, info.cnt, shape, tdt, 1e-3, info.sf, mode, qtable=q)
    idx, _ = ctx.ac_index(out, 64 * _nblk(shape))
    e = EDGE[len(shape)]
    lo = tuple(max(0, a - e - 1) for a in at)
    hi = tuple(min(d, a + e + 2) for a, d in zip(at, shape))
    want = _slice(full, shape, lo, hi).cpu().numpy()
    assert np.isnan(want).any() and not np.isnan(want).all()
    r = ctx.decompress_box_nd(out, info.cnt, shape, tdt, 1e-3, info.sf, lo, hi, idx, mode, qtable=q).cpu().numpy()
    assert NF.same_with_nans(r, want), NF.describe_mismatch(r, want)


def _raw(ctx, out, cnt, tdt, eb, sf, nd, dims, lo, hi, idx_ptr, mode, q, dst_ptr, bin_ptr=None, dc_ptr=None, ac_ptr=None):
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = lambda v: None if v is None else (C.c_size_t * len(v))(*v)
    return ctx.lib.dctzhip_decompress_box_nd(ctx.h, out["bin_index"].data_ptr() if bin_ptr is None else bin_ptr,
                                             out["dc"].data_ptr() if dc_ptr is None else dc_ptr,
                                             out["ac_exact"].data_ptr() if ac_ptr is None else ac_ptr, int(cnt), idx_ptr, qp, nd, arr(dims),
                                             H._dt(tdt), float(eb), float(sf), mode, arr(lo), arr(hi), dst_ptr)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == GAPS], ids=_id)
def test_refusals_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = _case(ctx, shape, kind, dtype, mode)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    n = int(np.prod(shape))
    dst = torch.empty(n + 2, dtype=tdt, device=ctx.device)
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    es = 8 if dtype == np.float64 else 4
    D, L, Hh = list(shape), [0, 20, 10], [12, 22, 200]
    ext = [h - l for l, h in zip(L, Hh)]
    want = _slice(full, shape, L, Hh)

    def call(nd=3, dims=D, lo=L, hi=Hh, ix=idx, cnt=info.cnt, dptr=None, qq=q, bptr=None, dcptr=None, acptr=None, ixptr=None):
        return _raw(ctx, cp, cnt, tdt, eb, info.sf, nd, dims, lo, hi, ix.data_ptr() if ixptr is None else ixptr, mode, qq,
                    dst.data_ptr() if dptr is None else dptr, bptr, dcptr, acptr)

    def after():
        assert call() == H.OK
        assert _same_dev(dst[:int(np.prod(ext))].view(ext), want)

    after()
    hit, t0, t1 = _hit_tiles(shape, L, Hh)
    th = np.flatnonzero(hit)
    big = 1 << 40
    host = [
        dict(nd=1, dims=D[:1], lo=L[:1], hi=Hh[:1]), dict(nd=4, dims=D + [1], lo=L + [0], hi=Hh + [1]), dict(nd=0), dict(nd=-1),
        dict(dims=None), dict(lo=None), dict(hi=None),
        dict(dims=[12, 0, 256]),                                                # a zero extent of the array
        dict(dims=[big, big, big], lo=[0, 0, 0], hi=[1, 1, 1]),                 # more blocks than an int of positions
        dict(lo=[0, 22, 10], hi=[12, 22, 200]), dict(lo=[0, 23, 10], hi=[12, 22, 200]),   # a zero / negative extent of the box
        dict(hi=[12, 22, 257]), dict(hi=[13, 22, 200]),
        dict(dptr=0), dict(dptr=dst.data_ptr() + es),                           # null / misaligned output
        dict(bptr=0), dict(bptr=cp["bin_index"].data_ptr() + 4),                # null / misaligned bin ids
        dict(dcptr=0), dict(dcptr=cp["dc"].data_ptr() + 2),                     # ... DC
        dict(ixptr=0), dict(ixptr=idx.data_ptr() + 2),                          # ... index
        dict(acptr=0), dict(acptr=cp["ac_exact"].data_ptr() + 2),               # null AC_exact with ac_count > 0 / misaligned
        dict(dptr=cp["bin_index"].data_ptr() + 4096 * int(th[1])),              # d_out over bin ids the call may read
        dict(dptr=idx.data_ptr() + 4 * int(th[0]) // 16 * 16),                  # ... over index entries
    ]
    if mode == H.QT:
        host.append(dict(qq=None))                                              # QT without its table
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
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
        assert _same_dev(dst[:int(np.prod(ext))].view(ext), want)
    # ac_count one short of what the last hit tile needs
    need = int(idx[int(th[-1]) + 1])
    assert need > 0 and info.cnt > 0
    assert call(cnt=need - 1) == H.E_ARG
    after()
    assert call(cnt=need) == H.OK
    assert _same_dev(dst[:int(np.prod(ext))].view(ext), want)
    for k in out:                                      # bit patterns: AC_exact beyond cnt is uninitialised (NaN != NaN)
        bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert torch.equal(bits(cp[k]), bits(out[k])), k
