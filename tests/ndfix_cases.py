"""The correction list of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h: dctzhip_fixup_build_nd), restated
in numpy from the definition, and the cases the CPU and GPU tests share.

Positions: the streams cover 64 nblk positions; position q belongs to block B = q >> 6 (row-major over the tile grid), its
in-block place is j = q & 63 (row-major inside the tile), its coordinate along axis a is e B_a + j_a.  A position is real iff
every coordinate is below the array's extent; the edge padding is never listed.  (oracle.nd_gather pads by REPEATING samples
and is not the tool for the listed mask: here the padding is False.)"""
import numpy as np

TILE = 4096
TILE_BLKS = 64
EDGE = {2: 8, 3: 4}
EB = 1e-3
MULTS = (0.25, 0.5, 1.0, 2.0, 4.0)
# what each shape is for: a tile with one block in it; ragged on every axis; a stream tile that wraps into the next block
# row; whole tiles; the same in 3-D; candidate tiles a thin box does not hit
SHAPES = [(8, 8), (45, 77), (16, 520), (64, 512), (4, 4, 4), (13, 22, 35), (16, 16, 32), (12, 64, 256)]
KINDS = ("smooth", "noisy")
BIG = (256, 256, 160)                 # 2560 stream tiles: more than a resident grid of single-wave workgroups


def field(shape, kind, dtype):
    """tests/test_gpu_fixup.py's _field(n, kind, dtype, seed=n), reshaped: sf = 100."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.float64)
    x = 100.0 + 60.0 * np.sin(i / 4000.0) + 6.0 * np.cos(i / 1000.0)
    if kind == "noisy":
        x = x + 25.0 * np.clip(np.random.default_rng(n).standard_normal(n), -4.0, 4.0)
    return np.ascontiguousarray(x.astype(dtype).reshape(shape))


def grid(shape):
    e = EDGE[len(shape)]
    return tuple(-(-d // e) for d in shape)


def nblk(shape):
    return int(np.prod(grid(shape)))


def tiles(shape):
    return -(-64 * nblk(shape) // TILE)


def has_full_tile(shape):
    return nblk(shape) >= TILE_BLKS


def coords(shape, q):
    """Array coordinates (one array per axis) of the stream positions q; they may lie beyond the extents."""
    nd, e = len(shape), EDGE[len(shape)]
    q = np.asarray(q, dtype=np.int64)
    b = np.unravel_index(q >> 6, grid(shape))
    j = np.unravel_index(q & 63, (e,) * nd)
    return tuple(e * b[a] + j[a] for a in range(nd))


def position(shape, c):
    """The stream position of the array coordinates c (one array or int per axis)."""
    e = EDGE[len(shape)]
    c = [np.asarray(v, dtype=np.int64) for v in c]
    b = np.ravel_multi_index([v // e for v in c], grid(shape))
    j = np.ravel_multi_index([v % e for v in c], (e,) * len(shape))
    return 64 * b + j


def real(shape):
    """bool per stream position: every coordinate inside the array."""
    c = coords(shape, np.arange(64 * nblk(shape)))
    ok = np.ones(64 * nblk(shape), bool)
    for a, d in enumerate(shape):
        ok &= c[a] < d
    return ok


def to_stream(shape, a, pad):
    """The array `a` in stream order, `pad` at the padded positions."""
    c = coords(shape, np.arange(64 * nblk(shape)))
    ok = real(shape)
    out = np.full(64 * nblk(shape), pad, dtype=a.dtype)
    out[ok] = a[tuple(v[ok] for v in c)]
    return out


def listed(x, r, bound):
    """bool array of x's shape: !(fabs(x - r) <= (T)bound), the difference taken in T."""
    assert x.dtype == r.dtype and x.shape == r.shape
    with np.errstate(invalid="ignore"):
        return ~(np.abs(x - r) <= x.dtype.type(bound))


def fix_list(x, r, bound):
    """(listed, fix_start uint32[tiles + 1], fix_off uint16[count], fix_val T[count]) of the definition."""
    shape = x.shape
    lm = listed(x, r, bound)
    ms = to_stream(shape, lm, False)
    m = tiles(shape)
    padded = np.zeros(m * TILE, bool)
    padded[:ms.size] = ms
    per = padded.reshape(m, TILE).sum(axis=1).astype(np.uint64)
    start = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    q = np.flatnonzero(ms)
    return lm, start, (q % TILE).astype(np.uint16), np.ascontiguousarray(x[coords(shape, q)])


def fix_list_loops(x, r, bound):
    """fix_list with plain loops over the positions (small shapes): pins the vectorised form."""
    shape = x.shape
    nd, e = len(shape), EDGE[len(shape)]
    g = grid(shape)
    b = x.dtype.type(bound)
    m = tiles(shape)
    per = [0] * m
    off, val = [], []
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
            if not (np.abs(x[c] - r[c]) <= b):
                per[q // TILE] += 1
                off.append(q % TILE)
                val.append(x[c])
    start = np.concatenate([[0], np.cumsum(np.array(per, dtype=np.uint64))]).astype(np.uint32)
    return start, np.array(off, dtype=np.uint16), np.array(val, dtype=x.dtype)


def applied(x, r, bound):
    return np.where(listed(x, r, bound), x, r)


def guarantee_holds(x, out, bound):
    """Every element has the bits of x or lies within (T)bound of it."""
    u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    same = np.ascontiguousarray(out).view(u) == np.ascontiguousarray(x).view(u)
    with np.errstate(invalid="ignore"):
        near = np.abs(x - out) <= x.dtype.type(bound)
    return bool((same | near).all())


def boxes(shape):
    """Corner boxes, boxes that cut blocks and tiles, one element, the last element; a box thin in y where the tiles are (z, y)
    block rows."""
    nd = len(shape)
    bx = [((0,) * nd, tuple(shape))]
    bx.append(((0,) * nd, tuple(max(1, d // 3) for d in shape)))
    bx.append((tuple(d - max(1, d // 3) for d in shape), tuple(shape)))
    bx.append((tuple(d // 4 for d in shape), tuple(max(d // 4 + 1, d - d // 4) for d in shape)))
    lo = [min(1, d - 1) for d in shape]
    hi = [max(l + 1, d - 1 - (d % 2 == 0 and d > 2)) for l, d in zip(lo, shape)]
    bx.append((tuple(lo), tuple(hi)))
    mid = tuple(d // 2 for d in shape)
    bx.append((mid, tuple(v + 1 for v in mid)))
    bx.append((tuple(d - 1 for d in shape), tuple(shape)))
    if shape == (12, 64, 256):
        bx += [((0, 20, 10), (12, 22, 200)), ((1, 63, 0), (9, 64, 256))]
    for lo, hi in bx:
        assert all(0 <= l < h <= d for l, h, d in zip(lo, hi, shape)), (lo, hi)
    return bx
