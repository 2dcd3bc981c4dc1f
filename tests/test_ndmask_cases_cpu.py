"""The numpy restatement of the tiled missing-value layer (tests/ndmask_cases.py) pinned against a plain per-tile loop on the
small shapes: padded positions are never sources, valid elements keep their bits, the filled array's max|x| is the valid
data's; and what the layer is for, on the CPU oracle: a field with 1e36 blobs compressed in tiles keeps the scaling factor of
its valid data once it is filled."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mask_cases as M
from tests import ndmask_cases as N


def _same_bits(a, b):
    U = M._bits(a.dtype)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("rule", sorted(M.RULES))
def test_fill_equals_the_plain_loop(dtype, rule):
    flags, value, limit = M.RULES[rule]
    for shape in N.shapes(dtype):
        for pat in N.PATTERNS:
            what = (shape, pat)
            x, want = N.build_input(shape, dtype, pat, rule)
            miss = M.is_missing(x, flags, value, limit)
            assert np.array_equal(miss, want), what               # markers are missing, specials are valid
            f = N.fill(x, miss)
            assert _same_bits(f, N.fill_loop(x, miss)), what
            assert _same_bits(f[~miss], x[~miss]), what           # valid elements untouched
            if rule != "value0":                                  # (value0 calls a tile's +0.0 missing again)
                assert not M.is_missing(f, flags, value, limit).any(), what
                assert _same_bits(N.fill(f, miss), f), what       # idempotent


def test_padded_positions_are_never_sources():
    """A ragged tile whose real part is all missing takes +0.0, whatever the edge padding would repeat; a missing position whose
    only predecessors in j are padded takes the tile's first real valid position."""
    for dtype in (np.float32, np.float64):
        for shape in ((9, 17), (13, 21), (5, 6, 7), (9, 4, 33)):
            x, miss = N.build_input(shape, dtype, "edge_tile_all", "value", with_specials=False)
            f = N.fill(x, miss)
            e = O.GEOM_EDGE[len(shape)]
            edge = tuple(slice((d - 1) // e * e, d) for d in shape)
            assert miss[edge].all() and (f[edge] == 0).all() and not np.signbit(f[edge]).any()
            assert _same_bits(f[~miss], x[~miss])
    # 2-D, extents (3, 5): j = 8 r + c; (1, 0) is missing, its predecessors j = 5 .. 7 are padded, j = 0 .. 4 valid -> takes (0, 4)
    x = np.arange(15, dtype=np.float64).reshape(3, 5) + 1
    miss = np.zeros((3, 5), bool)
    miss[1, 0] = True
    assert N.fill(x, miss)[1, 0] == x[0, 4]
    miss[:] = False
    miss[0, :3] = True                                            # a leading gap: the tile's first real valid position, (0, 3)
    assert (N.fill(x, miss)[0, :3] == x[0, 3]).all()


def test_the_fill_follows_the_tiles_not_the_rows():
    """Two 8 x 8 tiles side by side, the left one missing but for its last row: the flat fill would copy across the tile
    boundary, the tiled fill takes the left tile's own first valid position."""
    x = np.arange(128, dtype=np.float32).reshape(8, 16) + 1
    miss = np.zeros((8, 16), bool)
    miss[:7, :8] = True
    f = N.fill(x, miss)
    assert (f[:7, :8] == x[7, 0]).all() and _same_bits(f[~miss], x[~miss])
    flat = M.fill(x.reshape(-1), miss.reshape(-1)).reshape(8, 16)
    assert flat[1, 0] == x[0, 15]                                 # (what the flat rule does with the same array)


def test_filled_extremes_are_those_of_the_valid_data():
    for shape in ((24, 36), (12, 20, 36)):
        x, miss = N.build_input(shape, np.float64, "random30", "value", with_specials=False)
        f = N.fill(x, miss)
        assert miss.any() and not miss.all()
        assert np.abs(f).max() == np.abs(x[~miss]).max() and np.abs(f).min() == np.abs(x[~miss]).min()
        x, miss = N.build_input(shape, np.float64, "whole_tile", "value", with_specials=False)
        f = N.fill(x, miss)
        assert np.abs(f).max() == np.abs(x[~miss]).max() and np.abs(f).min() == 0.0      # the tile without a valid position


def test_mask_is_the_flat_mask_of_the_array_in_c_order():
    miss = N.pattern("checkerboard", (5, 6, 7))
    w = N.mask_words(miss)
    assert w.size == -(-210 // 64) and np.array_equal(M.mask_bits(w, 210), miss.reshape(-1)) and int(w[-1]) >> (210 % 64) == 0


def test_patterns_cover_what_they_name():
    for shape in ((24, 36), (12, 20, 36), (3, 5)):
        nd, e = len(shape), O.GEOM_EDGE[len(shape)]
        t = N.pattern("whole_tile", shape)
        assert t.sum() == np.prod([min(e, d) for d in shape][:-1]) * min(e, max(shape[-1] - e, 0) or shape[-1])
        lo = N.pattern("tile_last_only", shape)
        assert t.sum() - lo.sum() == 1
        assert N.pattern("tile_first_row", shape).sum() == min(e, max(shape[-1] - e, 0) or shape[-1])
        assert N.pattern("column_stripes", shape).all(axis=tuple(range(nd - 1))).sum() == (np.arange(shape[-1]) % 4 < 2).sum()
        c = N.pattern("checkerboard", shape)
        assert not c[(0,) * nd] and abs(int(c.sum()) * 2 - c.size) <= 1
        g = N.pattern("edge_tile_all", shape)
        assert g[(-1,) * nd] and g.sum() == np.prod([d - (d - 1) // e * e for d in shape])
    b = N.blobs((96, 160))
    assert 0.15 < b.mean() < 0.35


def test_a_tiled_field_with_1e36_blobs_keeps_the_scaling_factor_of_its_valid_data():
    shape = (96, 160)
    f = N.field(shape, np.float32)
    miss = N.blobs(shape)
    x = f.copy()
    x[miss] = 1e36
    assert O.compress_nd(x, 1e-3).sf == float(np.float32(1e35))
    filled = N.fill(x, miss)
    assert O.compress_nd(filled, 1e-3).sf == O.stats(x[~miss]).sf == 1.0
