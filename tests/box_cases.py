"""Workloads, boxes and checks of the box-decode tests for lists of boxes (tests/test_gpu_boxes_decode.py): the shapes, the
compressed cases (one compression per workload and module run), the boxes around every edge of a shape, the hit-tile mask
and the poisoning of everything a call must not read.  The definitions are those the single-box test was written with
(tests/test_gpu_box_decode.py); they live here so that the list tests do not depend on another test file."""
import itertools

import numpy as np

from tests import workloads as W
from dctz_amd import hip as H


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
