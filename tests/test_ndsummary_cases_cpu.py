"""The numpy restatement of the tiled tile summaries (tests/ndsummary_cases.py) against plain loops over the positions, and the
facts the GPU tests lean on: every tile of every shape holds a real position, and the tiles' real positions add up to the
array."""
import numpy as np
import pytest

from tests import ndsummary_cases as S

SMALL = [s for s in S.SHAPES if int(np.prod(s)) <= 50000]


def _pair(shape, dtype):
    """An original and a stand-in reconstruction: the original moved by a smooth offset within a few error bounds."""
    x = S.field(shape, "noisy", dtype)
    i = np.arange(x.size, dtype=np.float64).reshape(shape)
    full = (x.astype(np.float64) + 0.2 * np.sin(i / 7.0)).astype(dtype)
    return x, full


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_reduce_equals_the_loop_form(shape, dtype):
    x, full = _pair(shape, dtype)
    want, mag, m, wt, mt = S.reduce(shape, full, x)
    loops, ml = S.reduce_loops(shape, full, x)
    assert np.array_equal(m, ml)
    assert np.array_equal(_bits(want), _bits(loops))
    assert (mag[:, S.SUMS] >= np.abs(want[:, S.SUMS])).all()
    # the totals: extremes of the records, sums of the whole array
    assert wt[0] == want[:, 0].min() and wt[1] == want[:, 1].max() and wt[6] == want[:, 6].max()
    assert wt[4] == float(x.min()) and wt[5] == float(x.max())


def test_a_nan_is_passed_over_by_extremes_and_carried_by_sums():
    shape = (13, 22, 35)
    x, full = _pair(shape, np.float64)
    full[5, 6, 7] = np.nan
    t = int(S.position(shape, (5, 6, 7))) // S.TILE
    want, mag, m, wt, mt = S.reduce(shape, full, x)
    loops, _ = S.reduce_loops(shape, full, x)
    assert np.array_equal(_bits(want), _bits(loops))
    assert np.isnan(want[t, [2, 3, 7]]).all() and not np.isnan(want[t, list(S.EXTREMES)]).any()
    others = np.arange(want.shape[0]) != t
    assert not np.isnan(want[others]).any()


@pytest.mark.parametrize("shape", S.SHAPES + [S.BIG], ids=lambda s: "x".join(map(str, s)))
def test_every_tile_holds_a_real_position_and_they_add_up(shape):
    ok = S.real(shape)
    nt = S.tiles(shape)
    per = [int(ok[t * S.TILE:(t + 1) * S.TILE].sum()) for t in range(nt)]
    assert min(per) >= 1
    assert sum(per) == int(np.prod(shape))
    # ... because every block does
    assert ok.reshape(-1, 64).any(axis=1).all()
