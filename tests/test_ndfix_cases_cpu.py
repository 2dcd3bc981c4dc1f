"""CPU checks of tests/ndfix_cases.py: the numpy restatement of the tiled correction list against a plain-loop version, and the
case list's non-vacuity from the CPU oracle's compress_nd / decompress_nd -- for every shape, type, mode and both kinds the
count at 0.25 eb sf is > 0, the counts never increase with the multiple, the count at 4 eb sf is 0, and for the noisy field
on shapes with a full stream tile some tile lists more than half of its real positions.  Passes without the feature by
design: it guards the inputs of tests/test_gpu_ndfix.py."""
import numpy as np
import pytest

from tests import ndfix_cases as N


def test_the_field_is_the_flat_tests_field():
    from tests import test_gpu_fixup as F
    for shape in ((45, 77), (13, 22, 35)):
        n = int(np.prod(shape))
        for kind in N.KINDS:
            for dt in (np.float64, np.float32):
                assert np.array_equal(N.field(shape, kind, dt).reshape(-1), F._field(n, kind, dt, seed=n))
    assert N.EB == F.EB and N.MULTS == (0.25, 0.5, 1.0, 2.0, 4.0)


def test_case_list():
    assert N.SHAPES == [(8, 8), (45, 77), (16, 520), (64, 512), (4, 4, 4), (13, 22, 35), (16, 16, 32), (12, 64, 256)]
    assert [N.nblk(s) for s in N.SHAPES] == [1, 60, 130, 512, 1, 216, 128, 3 * 16 * 64]
    assert [N.has_full_tile(s) for s in N.SHAPES] == [False, False, True, True, False, True, True, True]
    assert N.nblk((16, 520)) % 64 != 0 and N.nblk((13, 22, 35)) % 64 != 0 and N.tiles(N.BIG) == 2560


@pytest.mark.parametrize("shape", N.SHAPES + [(9, 3), (1, 1, 1), (5, 9, 2)], ids=lambda s: "x".join(map(str, s)))
def test_position_and_coordinates(shape):
    n = 64 * N.nblk(shape)
    q = np.arange(n)
    c = N.coords(shape, q)
    ok = N.real(shape)
    assert int(ok.sum()) == int(np.prod(shape))
    assert np.array_equal(N.position(shape, [v[ok] for v in c]), q[ok])
    # every element once, and the in-block place is row-major inside the tile
    flat = np.ravel_multi_index([v[ok] for v in c], shape)
    assert np.array_equal(np.sort(flat), np.arange(int(np.prod(shape))))
    if len(shape) == 2:
        assert np.array_equal(q & 63, 8 * (c[0] % 8) + c[1] % 8)
    else:
        assert np.array_equal(q & 63, 16 * (c[0] % 4) + 4 * (c[1] % 4) + c[2] % 4)
    a = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    s = N.to_stream(shape, a, -1.0)
    assert (s[~ok] == -1.0).all() and np.array_equal(s[ok], flat.astype(np.float64))


@pytest.mark.parametrize("shape", [(8, 8), (45, 77), (16, 520), (4, 4, 4), (13, 22, 35)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_plain_loops_pin_the_vectorised_list(shape, dtype):
    rng = np.random.default_rng(7)
    x = N.field(shape, "noisy", dtype)
    r = (x + rng.normal(0.0, 0.1, shape)).astype(dtype)
    x[tuple(d // 2 for d in shape)] = np.nan                                    # a NaN in the original is listed
    r[tuple(d - 1 for d in shape)] = np.nan                                     # ... and one in the reconstruction
    for b in (0.0, 0.05, 0.1, 10.0):
        lm, start, off, val = N.fix_list(x, r, b)
        ls, lo, lv = N.fix_list_loops(x, r, b)
        assert np.array_equal(start, ls) and np.array_equal(off, lo)
        u = np.uint64 if dtype == np.float64 else np.uint32
        assert np.array_equal(val.view(u), lv.view(u))
        assert int(start[-1]) == int(lm.sum()) == off.size
        assert lm[tuple(d // 2 for d in shape)] and lm[tuple(d - 1 for d in shape)]
        assert N.guarantee_holds(x, N.applied(x, r, b), b)
    assert int(N.fix_list(x, r, 10.0)[1][-1]) == 2                               # the two NaNs alone


def test_boxes_are_inside_and_cut():
    for shape in N.SHAPES + [N.BIG]:
        bx = N.boxes(shape)
        assert bx[0] == ((0,) * len(shape), tuple(shape)) and bx[-1 if shape != (12, 64, 256) else -3][1] == tuple(shape)
    e = 4
    lo, hi = N.boxes((12, 64, 256))[-2]                                         # thin in y: (z, y) block rows between are not hit
    assert (hi[1] - 1) // e - lo[1] // e + 1 < 64 // e


CASES = [(s, dt, mode, kind) for s in N.SHAPES for dt in (np.float64, np.float32) for mode in (0, 1) for kind in N.KINDS]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}-{'x'.join(map(str, c[0]))}-{np.dtype(c[1]).name}-{'QT' if c[2] else 'EC'}")
def test_cases_are_not_vacuous(case):
    import oracle.oracle as O
    shape, dtype, mode, kind = case
    x = N.field(shape, kind, dtype)
    c = O.compress_nd(x, N.EB, O.QT if mode else O.EC)
    assert c.sf == 100.0
    r = O.decompress_nd(c, shape)
    counts = [int(N.fix_list(x, r, m * N.EB * c.sf)[1][-1]) for m in N.MULTS]
    print(f"{shape} {np.dtype(dtype).name} {'QT' if mode else 'EC'} {kind}: listed for m = {N.MULTS}: {counts}")
    assert counts[0] > 0
    assert counts == sorted(counts, reverse=True)
    assert counts[-1] == 0
    if kind == "noisy" and N.has_full_tile(shape):
        per = np.diff(N.fix_list(x, r, N.MULTS[0] * N.EB * c.sf)[1].astype(np.int64))
        reals = N.real(shape)
        rp = np.zeros(N.tiles(shape) * N.TILE, bool)
        rp[:reals.size] = reals
        rp = rp.reshape(-1, N.TILE).sum(axis=1)
        assert (2 * per > rp).any(), (per, rp)
