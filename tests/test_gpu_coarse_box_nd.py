"""A box of the coarse decode of an array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one call (include/dctz_hip.h:
dctzhip_decompress_coarse_box_nd): a window at zoom level f.

The yardstick is Context.decompress_coarse_nd, sliced, bit for bit (tests/test_gpu_coarse_decode.py holds that call to the
numpy low-band operator): no tolerance anywhere.  Locality (everything outside the HIT stream tiles is poisoned, candidate
tiles between hit ones included); output bounds (a guard around d_out); the DC-only form without the other streams; a NaN
block that the box straddles; the refusals, each followed by a good call; a corrupt index entry of a hit tile; one call on a
caller-selected stream directly behind its producers; the kernel's name.

Shapes: tests/test_gpu_ndbox_decode.py's, each the smallest at which one more thing can go wrong, plus (24, 1544): 193 blocks
per block row, so that a box thin in x leaves candidate tiles that are not hit in 2-D as well."""
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
FACTORS = {2: (2, 4, 8), 3: (2, 4)}
BIG = (256, 256, 160)                                  # 2560 stream tiles
GAPS3 = (12, 64, 256)                                  # a tile = one (z, y) block row: a box thin in y leaves candidate tiles that are not hit
GAPS2 = (24, 1544)                                     # 193 blocks per block row: three tiles and one block
RAGGED2, RAGGED3 = (45, 77), (13, 22, 35)
SHAPES = [(8, 8), (4, 4, 4), RAGGED2, RAGGED3, (16, 520), (64, 512), (16, 16, 32), GAPS3, GAPS2]
EBS = {"ragged": 1e-3, "dense": 1e-6, "none": 1e-1}
WORKLOADS = [(s, "ragged") for s in SHAPES] + [(RAGGED3, "dense"), (RAGGED3, "none")]
CASES = [(s, kind, dt, mode) for s, kind in WORKLOADS for dt in (np.float64, np.float32) for mode in (H.EC, H.QT)]


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


def _nb(shape):
    e = EDGE[len(shape)]
    return [-(-d // e) for d in shape]


def _nblk(shape):
    return int(np.prod(_nb(shape)))


def _cext(shape, f):
    return tuple(-(-d // f) for d in shape)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _tname(dtype):
    return "double" if dtype == np.float64 else "float"


def _kernel(shape, dtype, mode, f):
    K = EDGE[len(shape)] // f
    return f"k_ndcoarse_box_dc<{_tname(dtype)}>" if K == 1 else f"k_ndcoarse_box<{_tname(dtype)}, {mode}, {len(shape) - 1}, {K}>"


_CACHE = {}


def _compressed(ctx, x, eb, mode):
    """(out, info, index, eb, qtable, torch dtype, {factor: the whole coarse array}) of an array."""
    import torch
    tdt = _tdt(x.dtype.type)
    out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), eb, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    idx, tot = ctx.ac_index(out, 64 * _nblk(x.shape))
    assert tot == info.cnt
    coarse = {f: ctx.decompress_coarse_nd(out, info.cnt, x.shape, tdt, eb, info.sf, f, index=idx, mode=mode, qtable=q)
              for f in FACTORS[x.ndim]}
    return out, info, idx, eb, q, tdt, coarse


def _case(ctx, shape, kind, dtype, mode):
    """One workload, compressed once per module; the whole coarse arrays are computed once and never written again."""
    key = (shape, kind, np.dtype(dtype).name, mode)
    if key not in _CACHE:
        _CACHE[key] = _compressed(ctx, _input(shape, kind, dtype), EBS[kind], mode)
    return _CACHE[key]


def _ivw(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_dev(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(_ivw(a.contiguous()), _ivw(b.contiguous())))


def _slice(whole, lo, hi):
    return whole[tuple(slice(l, h) for l, h in zip(lo, hi))].contiguous()


def _box(ctx, data, shape, f, lo, hi, mode, out=None, idx=None, cnt=None, dst=None):
    o, info, ix, eb, q, tdt, _ = data
    return ctx.decompress_coarse_box_nd(o if out is None else out, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, f, lo, hi,
                                        index=ix if idx is None else idx, mode=mode, qtable=q, dst=dst)


# ---- boxes, in coarse coordinates --------------------------------------------------------------------------------------------
def _corners(cd):
    return [(tuple(c), tuple(v + 1 for v in c)) for c in itertools.product(*[sorted({0, d - 1}) for d in cd])]


def _clamped(cd, lo, hi):
    lo = [min(max(l, 0), d - 1) for l, d in zip(lo, cd)]
    hi = [min(max(h, l + 1), d) for l, h, d in zip(lo, hi, cd)]
    return tuple(lo), tuple(hi)


def _aligned(cd, nb, K):
    """On block boundaries on all sides (clamped to the coarse array where it is ragged)."""
    return _clamped(cd, [K * (b // 4) for b in nb], [K * max(b // 4 + 1, b - b // 4) for b in nb])


def _one_block(cd, K):
    org = [K * ((d - 1) // K // 2) for d in cd]
    return _clamped(cd, [o + (1 if K > 2 else 0) for o in org], [o + K for o in org])


def _odd_box(cd):
    """Fastest start and extent odd (where the axis has room), the other axes cut on both sides."""
    lo = [d // 4 for d in cd]
    hi = [max(l + 1, d - d // 4) for l, d in zip(lo, cd)]
    d = cd[-1]
    lo[-1] = min(1, d - 1)
    ext = max(1, min(d - lo[-1], 2 * (d // 3) + 1))
    ext -= 1 - ext % 2 if ext > 1 else 0
    hi[-1] = lo[-1] + ext
    return tuple(lo), tuple(hi)


def _far_corner(cd):
    """Ends at the last coarse cell of every axis: on a ragged shape it holds the cells that straddle the edge."""
    return tuple(d - max(1, d // 3) for d in cd), tuple(cd)


def _boxes(shape, f, seed, k=12):
    nd = len(shape)
    K = EDGE[nd] // f
    cd, nb = _cext(shape, f), _nb(shape)
    bx = [((0,) * nd, cd)] + _corners(cd)
    bx += [_aligned(cd, nb, K), _one_block(cd, K), _odd_box(cd), _far_corner(cd)]
    for a in range(nd):                                                               # a one-thick plane along every axis
        at = cd[a] // 3
        bx.append((tuple(at if i == a else 0 for i in range(nd)), tuple(at + 1 if i == a else cd[i] for i in range(nd))))
    rng = np.random.default_rng(seed + 31 * f + int(np.prod(shape)))
    for _ in range(k):                                                                # log-uniform extents
        ext = [max(1, min(d, int(np.exp(rng.uniform(0.0, np.log(d + 1)))))) for d in cd]
        lo = [int(rng.integers(0, d - x + 1)) for d, x in zip(cd, ext)]
        bx.append((tuple(lo), tuple(l + x for l, x in zip(lo, ext))))
    for lo, hi in bx:
        assert all(0 <= l < h <= d for l, h, d in zip(lo, hi, cd)), (lo, hi, cd)
    return bx


def test_boxes_are_what_they_claim():
    """(no GPU work) the aligned box starts on block boundaries, the single-block box lies inside one block, the odd box is
    odd, and on the ragged shapes the far corner holds a cell that straddles the array's edge."""
    for shape in SHAPES + [BIG]:
        for f in FACTORS[len(shape)]:
            K = EDGE[len(shape)] // f
            cd, nb = _cext(shape, f), _nb(shape)
            lo, hi = _aligned(cd, nb, K)
            assert all(l % K == 0 and (h % K == 0 or h == d) for l, h, d in zip(lo, hi, cd))
            lo, hi = _one_block(cd, K)
            assert all(l // K == (h - 1) // K for l, h in zip(lo, hi))
            lo, hi = _odd_box(cd)
            assert cd[-1] < 3 or (lo[-1] % 2 == 1 and (hi[-1] - lo[-1]) % 2 == 1)
            assert _far_corner(cd)[1] == cd
    for shape in (RAGGED2, RAGGED3):
        assert any(d % f for d in shape for f in FACTORS[len(shape)])                 # a last cell with fewer than f elements of its own


# ---- the box is the slice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_box_is_the_slice_of_the_coarse_decode(ctx, case):
    shape, kind, dtype, mode = case
    data = _case(ctx, shape, kind, dtype, mode)
    for f in FACTORS[len(shape)]:
        whole = data[6][f]
        assert tuple(whole.shape) == _cext(shape, f)
        for lo, hi in _boxes(shape, f, seed=5):
            r = _box(ctx, data, shape, f, lo, hi, mode)
            assert tuple(r.shape) == tuple(h - l for l, h in zip(lo, hi))
            assert _same_dev(r, _slice(whole, lo, hi)), (f, lo, hi)
        assert ctx.last_kernel(1) == _kernel(shape, dtype, mode, f)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_more_tiles_than_workgroups(dtype, monkeypatch):
    """(256, 256, 160), the whole coarse array as the box: 2560 candidate tiles.  A workgroup of k_ndcoarse_box is one wave
    with a few KiB of LDS, so a default context holds all 2560 at once; the context of this test is created under
    DCTZHIP_WG_PER_CU=8, which the call honours as the big kernels do: 2048 workgroups on 256 CUs, the grid-stride loop runs."""
    import dctz_amd
    monkeypatch.setenv("DCTZHIP_WG_PER_CU", "8")
    c = dctz_amd.Context(0)
    try:
        out, info, idx, eb, q, tdt, coarse = data = _compressed(c, _input(BIG, "ragged", dtype), EBS["ragged"], H.EC)
        cd = _cext(BIG, 2)
        r = _box(c, data, BIG, 2, (0, 0, 0), cd, H.EC)
        g, t = c.counter(11), c.counter(12)
        print(f"workgroups {g}, candidate tiles {t}")
        assert t == _nblk(BIG) // TILE_BLKS == 2560 and g < t
        assert c.last_kernel(1) == _kernel(BIG, dtype, H.EC, 2)
        assert _same_dev(r, coarse[2])
        lo, hi = (5, 50, 15), (10, 55, 75)                                            # ... and a box with runs of tiles that are not hit
        assert _same_dev(_box(c, data, BIG, 2, lo, hi, H.EC), _slice(coarse[2], lo, hi))
    finally:
        c.close()


# ---- locality ----------------------------------------------------------------------------------------------------------------
def _hit_tiles(shape, f, lo, hi):
    """From the contract: with K = edge / f the blocks [lo / K, (hi - 1) / K] per axis, a mask over the row-major block grid,
    64 blocks to a stream tile -> (hit per tile, t0, t1, first block, last block)."""
    K = EDGE[len(shape)] // f
    nb = _nb(shape)
    m = np.zeros(nb, bool)
    m[tuple(slice(l // K, (h - 1) // K + 1) for l, h in zip(lo, hi))] = True
    nblk = int(np.prod(nb))
    flat = np.zeros(-(-nblk // TILE_BLKS) * TILE_BLKS, bool)
    flat[:nblk] = m.reshape(-1)
    hit = flat.reshape(-1, TILE_BLKS).any(axis=1)
    t = np.flatnonzero(hit)
    b = np.flatnonzero(flat)
    return hit, int(t[0]), int(t[-1]) + 1, int(b[0]), int(b[-1])


def _poisoned(out, idx, nblk, hit, seed, dc_keep=None):
    """Copies of the streams and the index with everything the contract excludes overwritten.  dc_keep (the DC-only form): the
    blocks whose DC the call may read; nothing else of any stream is its to read."""
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
    bh[:nblk] = np.repeat(hit, TILE_BLKS)[:nblk] if dc_keep is None else dc_keep
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


# (shape, factor) -> boxes.  Those of GAPS2 and GAPS3 leave runs of candidate tiles that are not hit: asserted from the mask.
LOCAL_BOXES = {
    (GAPS2, 2): [((0, 0), (12, 8)), ((3, 700), (9, 772)), ((0, 771), (12, 772))],
    (GAPS2, 4): [((1, 1), (6, 4)), ((0, 380), (6, 386))],
    (GAPS2, 8): [((1, 1), (3, 2)), ((0, 0), (3, 2))],
    (GAPS3, 2): [((0, 4, 10), (6, 6, 20)), ((1, 31, 0), (5, 32, 128))],
    (GAPS3, 4): [((0, 2, 5), (3, 3, 10))],
    ((16, 520), 2): [((0, 0), (4, 4)), ((5, 250), (8, 260)), ((2, 100), (3, 101))],
    ((16, 520), 4): [((0, 0), (2, 2)), ((3, 125), (4, 130))],
    ((16, 520), 8): [((1, 60), (2, 65))],
    (RAGGED3, 2): [((0, 0, 0), (2, 4, 18)), ((6, 10, 17), (7, 11, 18)), ((2, 4, 1), (4, 6, 15))],
    (RAGGED3, 4): [((3, 5, 8), (4, 6, 9)), ((1, 2, 1), (3, 4, 8))],
}
LOCAL = [c for c in CASES if any(s == c[0] for s, _ in LOCAL_BOXES) and c[1] in ("ragged", "dense")]


def test_the_gap_boxes_leave_candidate_tiles_unhit():
    """(no GPU work) the hit model on the boxes of the two gap shapes: three hit tiles far apart."""
    hit, t0, t1, _, _ = _hit_tiles(GAPS2, 2, (0, 0), (12, 8))
    assert list(np.flatnonzero(hit)) == [0, 3, 6] and hit.size == 10 and int((~hit[t0:t1]).sum()) == 4
    hit, t0, t1, _, _ = _hit_tiles(GAPS2, 4, (1, 1), (6, 4))
    assert list(np.flatnonzero(hit)) == [0, 3, 6]
    hit, t0, t1, _, _ = _hit_tiles(GAPS3, 2, (0, 4, 10), (6, 6, 20))
    assert list(np.flatnonzero(hit)) == [2, 18, 34] and hit.size == 48 and int((~hit[t0:t1]).sum()) == 30
    hit, t0, t1, _, _ = _hit_tiles(GAPS3, 4, (0, 2, 5), (3, 3, 10))
    assert list(np.flatnonzero(hit)) == [2, 18, 34]


@pytest.mark.parametrize("case", LOCAL, ids=_id)
def test_box_reads_only_the_tiles_it_hits(ctx, case):
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = data = _case(ctx, shape, kind, dtype, mode)
    nblk = _nblk(shape)
    for f in FACTORS[len(shape)]:
        K = EDGE[len(shape)] // f
        for i, (lo, hi) in enumerate(LOCAL_BOXES[(shape, f)]):
            hit, t0, t1, bfirst, blast = _hit_tiles(shape, f, lo, hi)
            if K > 1 and shape in (GAPS2, GAPS3):
                assert (~hit[t0:t1]).sum() >= 2, (f, lo, hi)
            if K > 1:
                pout, pix = _poisoned(out, idx, nblk, hit, seed=i)
            else:                                      # the DC words from the first to the last block of the box; no tile of any other stream
                keep = np.zeros(nblk, bool)
                keep[bfirst:blast + 1] = True
                pout, pix = _poisoned(out, idx, nblk, np.zeros_like(hit), seed=i, dc_keep=keep)
            r = _box(ctx, data, shape, f, lo, hi, mode, out=pout, idx=pix)
            assert _same_dev(r, _slice(coarse[f], lo, hi)), (f, lo, hi)


# ---- output bounds -----------------------------------------------------------------------------------------------------------
GUARDED = [c for c in CASES if c[0] in ((8, 8), RAGGED2, (64, 512), RAGGED3, (16, 16, 32)) and c[1] == "ragged"]


@pytest.mark.parametrize("case", GUARDED, ids=_id)
def test_box_writes_only_its_output(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    data = _case(ctx, shape, kind, dtype, mode)
    tdt = data[5]
    G = 64                                             # guard elements on each side (keeps d_out 16-byte aligned)
    for f in FACTORS[len(shape)]:
        K = EDGE[len(shape)] // f
        cd = _cext(shape, f)
        for lo, hi in _corners(cd) + [_odd_box(cd), _aligned(cd, _nb(shape), K), _far_corner(cd), ((0,) * len(cd), cd)]:
            cnt = int(np.prod([h - l for l, h in zip(lo, hi)]))
            g = torch.empty(cnt + 2 * G, dtype=tdt, device=ctx.device)
            _ivw(g).fill_(0x5A5A5A5A)
            sentinel = g.clone()
            r = _box(ctx, data, shape, f, lo, hi, mode, dst=g[G:G + cnt])
            assert _same_dev(g[:G], sentinel[:G]) and _same_dev(g[G + cnt:], sentinel[G + cnt:]), (f, lo, hi)
            assert _same_dev(r, _slice(data[6][f], lo, hi)), (f, lo, hi)


# ---- the DC-only form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (RAGGED2, RAGGED3, GAPS2, GAPS3) and c[1] == "ragged"], ids=_id)
def test_dc_only_form_needs_the_dc_stream_alone(ctx, case):
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = _case(ctx, shape, kind, dtype, mode)
    f = EDGE[len(shape)]
    for lo, hi in _boxes(shape, f, seed=7, k=4):
        r = ctx.decompress_coarse_box_nd({"dc": out["dc"]}, 0, shape, tdt, eb, info.sf, f, lo, hi, index=None, mode=mode, qtable=q)
        assert _same_dev(r, _slice(coarse[f], lo, hi)), (lo, hi)
    assert ctx.last_kernel(1) == f"k_ndcoarse_box_dc<{_tname(dtype)}>"
    assert ctx.counter(12) == 0 and ctx.counter(11) >= 1


# ---- a NaN block -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RAGGED2, RAGGED3], ids=["45x77", "13x22x35"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_box_over_a_nan_block_is_the_slice(ctx, shape, dtype, mode):
    """A NaN in one block: a box that straddles the block is NaN exactly where the whole-array coarse call is NaN, and keeps
    the same bits everywhere else (tests/nonfinite.py's rule)."""
    x = _input(shape, "ragged", dtype)
    at = tuple(d // 2 for d in shape)
    x[at] = np.nan
    out, info, idx, eb, q, tdt, coarse = _compressed(ctx, x, 1e-3, mode)
    e = EDGE[len(shape)]
    for f in FACTORS[len(shape)]:
        K = e // f
        cd = _cext(shape, f)
        lo = tuple(max(0, a // f - K - 1) for a in at)
        hi = tuple(min(d, a // f + K + 2) for a, d in zip(at, cd))
        want = _slice(coarse[f], lo, hi).cpu().numpy()
        assert np.isnan(want).any() and not np.isnan(want).all(), f
        r = ctx.decompress_coarse_box_nd(out, info.cnt, shape, tdt, eb, info.sf, f, lo, hi, index=idx, mode=mode, qtable=q).cpu().numpy()
        assert NF.same_with_nans(r, want), (f, NF.describe_mismatch(r, want))


# ---- refusals and the index check --------------------------------------------------------------------------------------------
def _raw(ctx, out, cnt, tdt, eb, sf, nd, dims, f, lo, hi, idx_ptr, mode, q, dst_ptr, bin_ptr=None, dc_ptr=None, ac_ptr=None):
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = lambda v: None if v is None else (C.c_size_t * len(v))(*v)
    return ctx.lib.dctzhip_decompress_coarse_box_nd(ctx.h, out["bin_index"].data_ptr() if bin_ptr is None else bin_ptr,
                                                    out["dc"].data_ptr() if dc_ptr is None else dc_ptr,
                                                    out["ac_exact"].data_ptr() if ac_ptr is None else ac_ptr, int(cnt), idx_ptr, qp, nd,
                                                    arr(dims), H._dt(tdt), float(eb), float(sf), mode, int(f), arr(lo), arr(hi), dst_ptr)


REFUSE = {GAPS2: ((0, 0), (12, 8)), GAPS3: ((0, 4, 10), (6, 6, 20))}     # at factor 2: three hit tiles with gaps between them


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in REFUSE], ids=_id)
def test_refusals_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = _case(ctx, shape, kind, dtype, mode)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    nd = len(shape)
    dst = torch.empty(int(np.prod(shape)) + 2, dtype=tdt, device=ctx.device)
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    es = 8 if dtype == np.float64 else 4
    D, (L, Hh) = list(shape), [list(v) for v in REFUSE[shape]]
    ext = [h - l for l, h in zip(L, Hh)]
    want = _slice(coarse[2], L, Hh)
    cd = _cext(shape, 2)

    def call(nd=nd, dims=D, f=2, lo=L, hi=Hh, ix=idx, cnt=info.cnt, dptr=None, qq=q, bptr=None, dcptr=None, acptr=None, ixptr=None):
        return _raw(ctx, cp, cnt, tdt, eb, info.sf, nd, dims, f, lo, hi, ix.data_ptr() if ixptr is None else ixptr, mode, qq,
                    dst.data_ptr() if dptr is None else dptr, bptr, dcptr, acptr)

    def after():
        assert call() == H.OK
        assert _same_dev(dst[:int(np.prod(ext))].view(ext), want)

    after()
    hit, t0, t1, _, _ = _hit_tiles(shape, 2, L, Hh)
    th = np.flatnonzero(hit)
    one = [1] * nd
    host = [dict(f=v, lo=[0] * nd, hi=one) for v in (-2, 0, 1, 3, 6, 16, 64) + ((8,) if nd == 3 else ())]     # no such factor in this geometry
    host += [
        dict(nd=1, dims=D[:1], lo=L[:1], hi=Hh[:1]), dict(nd=4, dims=D + [1], lo=L + [0], hi=Hh + [1]), dict(nd=0), dict(dims=None),
        dict(lo=None), dict(hi=None),
        dict(lo=Hh), dict(lo=[h + 1 for h in Hh]),                               # a zero / negative extent of the box
        dict(lo=[0] * (nd - 1) + [Hh[-1]], hi=Hh),                               # ... along one axis
    ]
    for a in range(nd):                                                         # one past the coarse extent; the extent in ELEMENTS
        host.append(dict(lo=[0] * nd, hi=[cd[i] + 1 if i == a else cd[i] for i in range(nd)]))
        host.append(dict(lo=[0] * nd, hi=[shape[i] if i == a else cd[i] for i in range(nd)]))
    for v in FACTORS[nd][1:]:                                                   # what is inside at factor 2 is outside at a larger one
        host.append(dict(f=v, lo=[0] * nd, hi=list(cd)))
    host += [
        dict(dptr=0), dict(dptr=dst.data_ptr() + es),                           # null / misaligned output
        dict(bptr=0), dict(bptr=cp["bin_index"].data_ptr() + 4),                # null / misaligned bin ids
        dict(dcptr=0), dict(dcptr=cp["dc"].data_ptr() + 2),                     # ... DC
        dict(ixptr=0), dict(ixptr=idx.data_ptr() + 2),                          # ... index
        dict(acptr=0), dict(acptr=cp["ac_exact"].data_ptr() + 2),               # null AC_exact with ac_count > 0 / misaligned
        dict(dptr=cp["bin_index"].data_ptr() + 4096 * int(th[1])),              # d_out over a hit tile's bin ids
        dict(dptr=cp["bin_index"].data_ptr() + 4096 * (int(th[0]) + 1)),        # ... over a candidate tile's that is not hit
        dict(dptr=cp["ac_exact"].data_ptr()),                                   # ... over AC_exact
        dict(dptr=idx.data_ptr() + 4 * int(th[0]) // 16 * 16),                  # ... over index entries
        dict(f=EDGE[nd], lo=[0] * nd, hi=one, dptr=cp["dc"].data_ptr()),        # the DC-only form: over the DC word it reads
    ]
    if mode == H.QT:
        host.append(dict(qq=None))                                              # QT without its table
        host.append(dict(f=EDGE[nd], lo=[0] * nd, hi=one, qq=None))
    assert not hit[int(th[0]) + 1]
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    assert ctx.lib.dctzhip_decompress_coarse_box_nd(None, *([None] * 3), 0, None, None, nd, None, 0, 0.0, 0.0, 0, 2, None, None, None) == H.E_ARG
    # a corrupt index entry of a hit tile (its own entry, and the one behind it)
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


# ---- stream order ------------------------------------------------------------------------------------------------------------
def test_box_on_a_caller_stream_behind_its_producers(ctx):
    """compress_nd, ac_index and the box call on a stream of the caller's, nothing of the test's between them."""
    import torch
    shape, dtype, mode, f = RAGGED3, np.float64, H.EC, 2
    data = _case(ctx, shape, "ragged", dtype, mode)
    lo, hi = _odd_box(_cext(shape, f))
    want = _slice(data[6][f], lo, hi)
    xh = torch.from_numpy(_input(shape, "ragged", dtype)).pin_memory()
    s = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(s):
        x = xh.to(ctx.device, non_blocking=True)
        out, info = ctx.compress_nd(x, EBS["ragged"], mode)
        idx, tot = ctx.ac_index(out, 64 * _nblk(shape))
        r = ctx.decompress_coarse_box_nd(out, info.cnt, shape, _tdt(dtype), EBS["ragged"], info.sf, f, lo, hi, index=idx, mode=mode)
        keep = r.clone()
    s.synchronize()
    assert tot == info.cnt and _same_dev(keep, want)
    ctx._bind_stream()                                  # back on the default stream for the tests behind this one
