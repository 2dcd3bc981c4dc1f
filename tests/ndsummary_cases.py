"""Tile summaries of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h: dctzhip_tile_summary_nd), restated in
numpy from the definition, and what the CPU and GPU tests share.

Positions, shapes and fields are the tiled correction list's (tests/ndfix_cases.py): record t covers the REAL positions among
[4096 t, min(4096 (t + 1), 64 nblk)); a padded position enters no field.  Extremes pass a NaN over (an all-NaN tile reports
+DBL_MAX / -DBL_MAX, emax 0); sums are math.fsum of the exact double terms and NaN as soon as one term is."""
import math

import numpy as np

from tests.ndfix_cases import BIG, EB, KINDS, SHAPES, TILE, coords, field, grid, nblk, position, real, tiles, to_stream  # noqa: F401

U = 2.0 ** -53
DBL_MAX = float(np.finfo(np.float64).max)
FIELDS = ("rmin", "rmax", "rsum", "rsq", "xmin", "xmax", "emax", "esq")
EXTREMES, SUMS = (0, 1, 4, 5, 6), (2, 3, 7)


def _passing_min(v):
    v = v[~np.isnan(v)]
    return float(v.min()) if v.size else DBL_MAX


def _passing_max(v, start):
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else start


def _one(r, x, e):
    """The eight fields of the elements r (reconstruction), x (original), e = x - r in the data type, and the sums of |term|."""
    rd, xd = r.astype(np.float64), x.astype(np.float64)
    terms = {2: rd, 3: rd * rd, 7: (e * e).astype(np.float64)}
    w, m = np.zeros(8), np.zeros(8)
    w[0], w[4] = _passing_min(rd), _passing_min(xd)
    w[1], w[5] = _passing_max(rd, -DBL_MAX), _passing_max(xd, -DBL_MAX)
    w[6] = _passing_max(np.abs(e).astype(np.float64), 0.0)
    for f, t in terms.items():
        w[f] = math.nan if np.isnan(t).any() else math.fsum(t.tolist())
        m[f] = w[f] if (t >= 0).all() else math.fsum(np.abs(t).tolist())
    return w, m


def reduce(shape, full, x):
    """-> (want (tiles, 8), mag (tiles, 8), m (tiles,), want_total (8,), mag_total (8,)): the fields per stream tile and over the
    array from the full decode `full` and the original `x` (both of `shape`), over real positions only; mag: the sums of
    |term| of the three sums; m: the real positions of each tile."""
    assert full.shape == tuple(shape) == x.shape and full.dtype == x.dtype
    with np.errstate(invalid="ignore"):
        e = x - full                                      # in the array's dtype
    # to_stream() of the three arrays, the coordinates taken once
    c = coords(shape, np.arange(64 * nblk(shape)))
    ok = np.ones(64 * nblk(shape), bool)
    for a, d in enumerate(shape):
        ok &= c[a] < d
    at = tuple(v[ok] for v in c)
    fs, xs, es = (np.zeros(ok.size, full.dtype) for _ in range(3))
    fs[ok], xs[ok], es[ok] = full[at], x[at], e[at]
    nt = tiles(shape)
    want, mag, m = np.zeros((nt, 8)), np.zeros((nt, 8)), np.zeros(nt, np.int64)
    for t in range(nt):
        sl = slice(t * TILE, min(t * TILE + TILE, ok.size))
        k = ok[sl]
        m[t] = int(k.sum())
        want[t], mag[t] = _one(fs[sl][k], xs[sl][k], es[sl][k])
    wt, mt = _one(full.reshape(-1), x.reshape(-1), e.reshape(-1))
    return want, mag, m, wt, mt


def reduce_loops(shape, full, x):
    """reduce()'s per-tile part with plain loops over the positions (small shapes): pins the vectorised form."""
    nd, e = len(shape), {2: 8, 3: 4}[len(shape)]
    g = grid(shape)
    nt = tiles(shape)
    vals = [([], [], []) for _ in range(nt)]
    for q in range(64 * nblk(shape)):
        B, j = q >> 6, q & 63
        c = []
        for a in range(nd - 1, -1, -1):
            c.append(e * (B % g[a]) + j % e)
            B //= g[a]
            j //= e
        c = tuple(reversed(c))
        if any(v >= d for v, d in zip(c, shape)):
            continue
        with np.errstate(invalid="ignore"):
            vals[q // TILE][0].append(full[c]); vals[q // TILE][1].append(x[c]); vals[q // TILE][2].append(x[c] - full[c])
    want, m = np.zeros((nt, 8)), np.zeros(nt, np.int64)
    for t, (r, o, d) in enumerate(vals):
        m[t] = len(r)
        rmin, rmax, xmin, xmax, emax = DBL_MAX, -DBL_MAX, DBL_MAX, -DBL_MAX, 0.0
        tr, tq, te = [], [], []
        for rv, ov, dv in zip(r, o, d):
            rf, of = float(rv), float(ov)
            if not math.isnan(rf):
                rmin, rmax = min(rmin, rf), max(rmax, rf)
            if not math.isnan(of):
                xmin, xmax = min(xmin, of), max(xmax, of)
            if not math.isnan(float(dv)):
                emax = max(emax, abs(float(dv)))
            tr.append(rf); tq.append(rf * rf); te.append(float(dv * dv))
        s = [math.nan if any(math.isnan(v) for v in tt) else math.fsum(tt) for tt in (tr, tq, te)]
        want[t] = [rmin, rmax, s[0], s[1], xmin, xmax, emax, s[2]]
    return want, m


def bound(m, mag):
    """|any-order sum of m doubles - their exact sum| <= (m - 1) u / (1 - (m - 1) u) sum |t_i|, u = 2^-53."""
    return (m - 1) * U / (1.0 - (m - 1) * U) * mag
