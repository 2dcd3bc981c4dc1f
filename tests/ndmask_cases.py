"""The missing-value layer of arrays compressed in 8 x 8 / 4 x 4 x 4 tiles restated in numpy (include/dctz_hip.h, "missing values
of an array compressed in ... tiles"): the fill inside each tile in ascending in-tile place j, over the real positions alone,
vectorised -- the array, the "real" map and the "missing" map gathered to (nblk, 64) in the oracle's nd_gather layout -- and the
case list the tests share: shapes, patterns of missing elements, and the inputs built from them.  The tests for "missing", the
mask words, the rules, markers and special values are those of tests/mask_cases.py."""
import numpy as np

from oracle import oracle as O
from tests import mask_cases as M

F32, F64 = np.float32, np.float64

# the smallest shapes at which each path of the kernel can go wrong: one element, one ragged tile, one whole tile, one full trip
# (E = 2 fp64 / 4 fp32 tiles along the last axis), a last extent that is a multiple of the tile but not of a trip, odd extents,
# an odd pitch (element path), a pitch of whole 16 bytes with ragged tiles, several trips of several waves
SHAPES_2D = {F64: ((1, 1), (3, 5), (8, 8), (8, 16), (16, 40), (9, 17), (13, 21), (24, 36), (64, 96)),
             F32: ((1, 1), (3, 5), (8, 8), (8, 32), (16, 40), (9, 17), (13, 21), (24, 36), (64, 96))}
SHAPES_3D = ((1, 1, 1), (4, 4, 4), (4, 4, 8), (8, 8, 16), (5, 6, 7), (9, 4, 33), (12, 20, 36))
# one per geometry beyond num_cu * 8 workgroups of the grid-stride loop (over 32 MiB), ragged in every axis
BIG = (((2051, 2309), F64), ((203, 211, 229), F32))


def shapes(dtype):
    return SHAPES_2D[np.dtype(dtype).type] + SHAPES_3D


def _tiles(a, cval):
    """(nblk, 64): the array tile after tile, row-major inside a tile; padded positions hold cval."""
    e = O.GEOM_EDGE[a.ndim]
    ap = np.pad(a, [(0, (-d) % e) for d in a.shape], mode="constant", constant_values=cval)
    return O.nd_gather(ap).reshape(-1, 64)


def fill(x, miss):
    """The filled array: a real missing position takes the nearest real valid position before it in its tile (ascending j), else
    the tile's first real valid position, else +0.0.  Values move as bit patterns."""
    U = M._bits(x.dtype)
    xb = _tiles(np.ascontiguousarray(x).view(U), U(0))
    valid = _tiles(np.ones(x.shape, bool), False) & ~_tiles(miss, False)        # real and not missing
    j = np.arange(64)
    prev = np.maximum.accumulate(np.where(valid, j, -1), axis=1)               # place of the last valid position at or before j
    first = np.argmax(valid, axis=1)                                          # place of the first valid position (0 if none)
    src = np.where(prev >= 0, prev, first[:, None])
    got = np.take_along_axis(xb, src, axis=1)
    out = np.where(valid.any(axis=1)[:, None], got, U(0))
    return O.nd_scatter(out.reshape(-1), x.shape).view(x.dtype)


def fill_loop(x, miss):
    """The same rule as a plain loop over tiles and places (small arrays only: what pins fill())."""
    e = O.GEOM_EDGE[x.ndim]
    out = x.copy()
    ob = out.view(M._bits(x.dtype))
    for origin in np.ndindex(*[-(-d // e) for d in x.shape]):
        places = [tuple(o * e + c for o, c in zip(origin, cell)) for cell in np.ndindex(*([e] * x.ndim))]      # ascending j
        real = [p for p in places if all(c < d for c, d in zip(p, x.shape))]
        valid = [k for k, p in enumerate(real) if not miss[p]]
        for k, p in enumerate(real):
            if miss[p]:
                before = [v for v in valid if v < k]
                ob[p] = ob[real[before[-1]]] if before else ob[real[valid[0]]] if valid else 0
    return out


def mask_words(miss):
    return M.mask_words(np.ascontiguousarray(miss).reshape(-1))


# ---- patterns of missing elements: name -> boolean array of `shape` ----
ND_PATTERNS = ("whole_tile", "tile_last_only", "tile_first_row", "column_stripes", "checkerboard", "edge_tile_all")
PATTERNS = M.PATTERNS + ND_PATTERNS           # ("none" and "all" are among the flat ones)


def pattern(name, shape):
    if name in M.PATTERNS:                    # over the flattened array: runs that cross rows and tiles
        return M.pattern(name, int(np.prod(shape))).reshape(shape)
    nd, e = len(shape), O.GEOM_EDGE[len(shape)]
    m = np.zeros(shape, bool)
    # the second tile along the last axis where there is one (valid tiles on either side in the wider shapes), else the first
    x0 = e if shape[-1] > e else 0
    tile = tuple(slice(0, e) for _ in range(nd - 1)) + (slice(x0, x0 + e),)
    if name == "whole_tile":
        m[tile] = True
    elif name == "tile_last_only":            # a leading gap of 63 places (fewer in a ragged tile)
        m[tile] = True
        m[tuple(min(s.stop, d) - 1 for s, d in zip(tile, shape))] = False
    elif name == "tile_first_row":
        m[(0,) * (nd - 1) + (tile[-1],)] = True
    elif name == "column_stripes":
        m[..., np.arange(shape[-1]) % 4 < 2] = True
    elif name == "checkerboard":
        m = np.indices(shape).sum(axis=0) % 2 == 1
    elif name == "edge_tile_all":             # the last tile along every axis: all of its real part
        m[tuple(slice((d - 1) // e * e, d) for d in shape)] = True
    else:
        raise KeyError(name)
    return m


def build_input(shape, dtype, pat, rule, with_specials=True):
    """(x, miss) of `shape`: mask_cases.build_input with the pattern taken over the array."""
    dtype = np.dtype(dtype).type
    n = int(np.prod(shape))
    miss = pattern(pat, shape).reshape(-1)
    U = M._bits(dtype)
    x = M.smooth(n, dtype, seed=n % 1000)
    if with_specials:
        sp = M.specials(rule, dtype)
        at = np.flatnonzero(~miss)[::11]
        x.view(U)[at] = np.resize(sp.view(U), at.size)
    at = np.flatnonzero(miss)
    x.view(U)[at] = np.resize(M.markers(rule, dtype).view(U), at.size)
    return x.reshape(shape), miss.reshape(shape)


def blobs(shape, threshold=0.3):
    """Smooth blobs over about a third of the array, a few tiles wide, so that the small shapes have them too."""
    g = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in shape], indexing="ij", sparse=True)
    f = np.sin(g[-1] / 7.0 + 0.5) * np.cos(g[-2] / 5.0) + 0.6 * np.sin((g[-1] + 2.0 * g[-2]) / 11.0)
    if len(shape) == 3:
        f = f + 0.5 * np.sin(g[0] / 3.0 + 1.0)
    return f > threshold


def field(shape, dtype):
    """Smooth finite data of magnitude below 10 (sf = 1) that varies along every axis."""
    g = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in shape], indexing="ij", sparse=True)
    f = 3.0 + 2.0 * np.sin(g[-1] / 29.0) + 1.5 * np.cos(g[-2] / 19.0)
    if len(shape) == 3:
        f = f + np.sin(g[0] / 11.0)
    rng = np.random.default_rng(int(np.prod(shape)) % 1000)
    return np.ascontiguousarray((f + 0.01 * rng.standard_normal(shape)).astype(dtype))
