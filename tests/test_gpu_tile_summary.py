"""Tile summaries (include/dctz_hip.h: dctzhip_tile_summary): one record per 4096-element tile of what dctzhip_decompress
would write -- min, max, sum, sum of squares -- and, with the original, min / max of the original, max |x - r| and
sum (x - r)^2, without the reconstruction ever being written.

Reference: the library's own ctx.decompress of the same streams, reduced tile by tile in numpy.
  * extremes (rmin, rmax, xmin, xmax, emax) are equal as bits; e = x - r is formed in the array's dtype;
  * a sum S over m terms t_i -- exact doubles: (double)r, (double)r * (double)r, the product e * e of the data type widened
    -- lies within (m - 1) u / (1 - (m - 1) u) sum |t_i| of math.fsum(t), u = 2^-53: the standard bound for ANY order of
    summation of m terms, not a measured number.  For a tile of 4096 values near 100 the bound is about 2e-7 on rsum; one
    coefficient off by one bin moves rsum by about 2 eb alpha_64 sf = 0.035 at sf = 100: a wrong value cannot hide.
"""
import ctypes as C
import math

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import nonfinite as NF

pytestmark = pytest.mark.gpu

EB = 1e-3
TILE = 4096
U = 2.0 ** -53
DBL_MAX = float(np.finfo(np.float64).max)
FLAT_N = [37, 4096, 4097, 3 * 4096 + 5 * 64 + 37]
BIG_N = 2051 * 4096 + 100            # above any resident grid of single-wave workgroups on 256 CUs: the grid-stride loop
CASES = [(n, dt, mode, kind) for n in FLAT_N for dt in (np.float64, np.float32) for mode in (H.EC, H.QT) for kind in ("smooth", "noisy")]
FIELDS = ("rmin", "rmax", "rsum", "rsq", "xmin", "xmax", "emax", "esq")
EXTREMES, SUMS = (0, 1, 4, 5, 6), (2, 3, 7)


def _id(c):
    n, dt, mode, kind = c
    return f"{kind}-{n}-{np.dtype(dt).name}-{'QT' if mode == H.QT else 'EC'}"


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _field(n, kind, dtype, seed):
    """The scaled samples are x / sf with sf the power of ten below max |x| (100 here: 100 < max |x| <= 1000, so the de-scale
    multiply runs); a coefficient beyond 255 eb = 0.255 is stored exactly.  smooth: a scaled block rises by at most 0.014 --
    nothing is stored exactly.  noisy: white noise of scaled sigma = 0.25 on top: about three coefficients in ten are stored
    exactly, at every position (both asserted where they are used)."""
    i = np.arange(n, dtype=np.float64)
    x = 100.0 + 60.0 * np.sin(i / 4000.0) + 6.0 * np.cos(i / 1000.0)
    if kind == "noisy":
        x = x + 25.0 * np.clip(np.random.default_rng(seed).standard_normal(n), -4.0, 4.0)
    return x.astype(dtype)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _streams(ctx, x, mode):
    """(device original, out, info, full decode (numpy), index, qtable) of one array."""
    import torch
    xd = torch.from_numpy(x).to(ctx.device)
    out, info = ctx.compress(xd, EB, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress(out, info.cnt, x.size, _tdt(x.dtype.type), EB, info.sf, mode, qtable=q).cpu().numpy()
    idx, tot = ctx.ac_index(out, x.size)
    assert tot == info.cnt
    return xd, out, info, full, idx, q


def _passing_min(v):
    v = v[~np.isnan(v)]
    return float(v.min()) if v.size else DBL_MAX


def _passing_max(v, start):
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else start


def _reduce(full, x):
    """Per tile and over the whole array: the eight fields from the full decode (sums by math.fsum) and the sums of |term|.
    -> (want (tiles, 8), mag (tiles, 8), want_total (8), mag_total (8))"""
    n = full.size
    r = full.astype(np.float64)
    e = (x - full)                                        # in the array's dtype
    terms = {2: r, 3: r * r, 7: (e * e).astype(np.float64)}
    ext = {0: r, 1: r, 4: x.astype(np.float64), 5: x.astype(np.float64), 6: np.abs(e).astype(np.float64)}

    def one(lo, hi):
        w, m = np.zeros(8), np.zeros(8)
        w[0], w[4] = _passing_min(ext[0][lo:hi]), _passing_min(ext[4][lo:hi])
        w[1], w[5] = _passing_max(ext[1][lo:hi], -DBL_MAX), _passing_max(ext[5][lo:hi], -DBL_MAX)
        w[6] = _passing_max(ext[6][lo:hi], 0.0)
        for f, t in terms.items():
            w[f] = math.fsum(t[lo:hi]) if not np.isnan(t[lo:hi]).any() else math.nan
            m[f] = w[f] if (t[lo:hi] >= 0).all() else math.fsum(np.abs(t[lo:hi]))
        return w, m

    tiles = -(-n // TILE)
    want, mag = np.zeros((tiles, 8)), np.zeros((tiles, 8))
    for t in range(tiles):
        want[t], mag[t] = one(t * TILE, min(t * TILE + TILE, n))
    wt, mt = one(0, n)
    return want, mag, wt, mt


def _bound(m, mag):
    return (m - 1) * U / (1.0 - (m - 1) * U) * mag


def _check(recs, total, want, mag, wt, mt, n, with_ref, what):
    """recs (tiles, 8) numpy, total a TileSummary, against _reduce's output."""
    tiles = -(-n // TILE)
    assert recs.shape == (tiles, 8), what
    tot = np.array([getattr(total, f) for f in FIELDS])
    if not with_ref:
        assert not recs[:, 4:].any() and not tot[4:].any(), what      # +0.0 in all four
        assert not _bits(recs[:, 4:]).any() and not _bits(tot[4:]).any(), what
    fields_e = [f for f in EXTREMES if with_ref or f < 4]
    fields_s = [f for f in SUMS if with_ref or f < 4]
    for f in fields_e:
        assert np.array_equal(_bits(recs[:, f]), _bits(want[:, f])), (what, FIELDS[f])
    worst = 0.0
    for t in range(tiles):
        m = min(t * TILE + TILE, n) - t * TILE
        for f in fields_s:
            b = _bound(m, mag[t, f])
            err = abs(recs[t, f] - want[t, f])
            worst = max(worst, err / b if b else (0.0 if err == 0 else math.inf))
            assert err <= b, (what, t, FIELDS[f], recs[t, f], want[t, f], b)
    print(f"{what}: worst |sum - fsum| / bound over the records = {worst:.3g}")
    # the total: extremes of the records, sums within the bound of m = n terms
    for f in fields_e:
        pick = np.min if f in (0, 4) else np.max
        assert _bits(tot[f:f + 1])[0] == _bits(np.array([pick(recs[:, f])]))[0], (what, FIELDS[f])
        assert _bits(tot[f:f + 1])[0] == _bits(wt[f:f + 1])[0], (what, FIELDS[f])
    for f in fields_s:
        b = _bound(n, mt[f])
        print(f"{what}: total {FIELDS[f]} = {tot[f]!r}, fsum = {wt[f]!r}, bound = {b:.3g}")
        assert abs(tot[f] - wt[f]) <= b, (what, FIELDS[f], tot[f], wt[f], b)


_DATA = {}


def _data(ctx, n, dtype, mode, kind):
    key = (n, np.dtype(dtype).name, mode, kind)
    if key not in _DATA:
        x = _field(n, kind, dtype, seed=n)
        s = _streams(ctx, x, mode)
        _DATA[key] = (x,) + s + _reduce(s[3], x)
    return _DATA[key]


def _flag_fraction(out, n):
    b = out["bin_index"].cpu().numpy()[:n // 64 * 64].reshape(-1, 64)[:, 1:]
    return float((b == 255).mean())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_records_are_the_reductions_of_the_full_decode(ctx, case):
    n, dtype, mode, kind = case
    x, xd, out, info, full, idx, q, want, mag, wt, mt = _data(ctx, n, dtype, mode, kind)
    tdt = _tdt(dtype)
    assert info.sf == 100.0                               # the de-scale multiply runs
    if n >= 4096:
        p = _flag_fraction(out, n)
        assert p == 0.0 if kind == "smooth" else 0.2 < p < 0.4, p
    tn = "double" if dtype == np.float64 else "float"
    for ref in (None, xd):
        what = f"{_id(case)} ref={ref is not None}"
        recs, total = ctx.tile_summary(out, info.cnt, n, tdt, EB, info.sf, index=idx, mode=mode, qtable=q, ref=ref)
        kern = "k_tile_summary" if n >= 64 else "k_tile_summary_rem"
        assert ctx.last_kernel(1) == f"{kern}<{tn}, {mode}, {'true' if ref is not None else 'false'}>"
        r1 = recs.cpu().numpy()
        _check(r1, total, want, mag, wt, mt, n, ref is not None, what)
        if ref is not None:
            pt = np.array(ctx.psnr_terms(xd, ctx.decompress(out, info.cnt, n, tdt, EB, info.sf, mode, qtable=q)))
            got = np.array([total.xmin, total.xmax, total.emax])
            assert np.array_equal(_bits(got), _bits(pt[:3])), (what, got, pt)
            assert abs(total.esq - pt[3]) <= _bound(n, mt[7]), (what, total.esq, pt[3])
            assert total.psnr(n) == 20.0 * np.log10((total.xmax - total.xmin) / np.sqrt(total.esq / n))
        # the same call twice: the same bytes in every record and in the total; index=None builds the index itself
        recs2, total2 = ctx.tile_summary(out, info.cnt, n, tdt, EB, info.sf, mode=mode, qtable=q, ref=ref)
        assert np.array_equal(_bits(recs2.cpu().numpy()), _bits(r1)), what
        assert bytes(total2) == bytes(total), what


@pytest.mark.parametrize("case", [(FLAT_N[-1], np.float64, H.EC, "noisy"), (FLAT_N[-1], np.float32, H.QT, "noisy")], ids=_id)
def test_a_second_context_gives_the_same_bytes(ctx, case):
    import dctz_amd
    n, dtype, mode, kind = case
    x, xd, out, info, full, idx, q, *_ = _data(ctx, n, dtype, mode, kind)
    other = dctz_amd.Context(0)
    try:
        for ref in (None, xd):
            a, ta = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, mode=mode, qtable=q, ref=ref)
            b, tb = other.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, mode=mode, qtable=q, ref=ref)
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
            assert bytes(ta) == bytes(tb)
    finally:
        other.close()


def test_more_tiles_than_resident_workgroups(ctx):
    """2052 tiles: a workgroup of the main kernel takes several (the grid-stride loop), the last tile is partial and holds a
    short block, and k_tile_summary_final runs three levels."""
    n, dtype, mode = BIG_N, np.float64, H.EC
    x = _field(n, "noisy", dtype, seed=7)
    xd, out, info, full, idx, q = _streams(ctx, x, mode)
    want, mag, wt, mt = _reduce(full, x)
    for ref in (None, xd):
        recs, total = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, mode=mode, ref=ref)
        _check(recs.cpu().numpy(), total, want, mag, wt, mt, n, ref is not None, f"big ref={ref is not None}")


def test_total_alone_and_records_alone(ctx):
    """d_tiles == NULL keeps the records in scratch of the context; total == NULL joins nothing."""
    import torch
    n, dtype, mode = FLAT_N[-1], np.float64, H.EC
    x, xd, out, info, full, idx, q, *_ = _data(ctx, n, dtype, mode, "noisy")
    recs, total = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, ref=xd)

    def raw(tiles_ptr, total_ref):
        return ctx.lib.dctzhip_tile_summary(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(info.cnt),
                                            idx.data_ptr(), None, n, H.F64, EB, float(info.sf), mode, xd.data_ptr(), tiles_ptr, total_ref)

    t2 = H.TileSummary()
    assert raw(None, C.byref(t2)) == H.OK and bytes(t2) == bytes(total)
    r2 = torch.zeros_like(recs)
    assert raw(r2.data_ptr(), None) == H.OK
    assert np.array_equal(_bits(r2.cpu().numpy()), _bits(recs.cpu().numpy()))
    assert raw(None, None) == H.E_ARG


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_refusals_leave_the_context_usable(ctx, dtype, mode):
    import torch
    n = FLAT_N[-1]
    x, xd, out, info, full, idx, q, *_ = _data(ctx, n, dtype, mode, "noisy")
    if q is not None:
        q = np.ascontiguousarray(q, dtype=dtype)
    tdt = _tdt(dtype)
    es = 8 if dtype == np.float64 else 4
    good, good_total = ctx.tile_summary(out, info.cnt, n, tdt, EB, info.sf, index=idx, mode=mode, qtable=q, ref=xd)
    recs = torch.zeros_like(good)
    total = H.TileSummary()

    def call(nn=n, cnt=info.cnt, ixptr=None, qq=q, refptr=None, tptr=None, bptr=None, dcptr=None, acptr=None):
        return ctx.lib.dctzhip_tile_summary(
            ctx.h, out["bin_index"].data_ptr() if bptr is None else bptr, out["dc"].data_ptr() if dcptr is None else dcptr,
            out["ac_exact"].data_ptr() if acptr is None else acptr, int(cnt), idx.data_ptr() if ixptr is None else ixptr,
            qq.ctypes.data_as(C.c_void_p) if qq is not None else None, nn, H._dt(tdt), EB, float(info.sf), mode,
            xd.data_ptr() if refptr is None else refptr, recs.data_ptr() if tptr is None else tptr, C.byref(total))

    def after():
        assert call() == H.OK
        assert np.array_equal(_bits(recs.cpu().numpy()), _bits(good.cpu().numpy())) and bytes(total) == bytes(good_total)

    after()
    host = [dict(nn=0),
            dict(bptr=0), dict(bptr=out["bin_index"].data_ptr() + 4), dict(dcptr=0), dict(dcptr=out["dc"].data_ptr() + 2),
            dict(ixptr=0), dict(ixptr=idx.data_ptr() + 2), dict(acptr=0), dict(acptr=out["ac_exact"].data_ptr() + 2),
            dict(refptr=xd.data_ptr() + es),                                    # the original not 16-byte aligned
            dict(tptr=recs.data_ptr() + 4),                                     # the records not 8-byte aligned
            dict(tptr=out["bin_index"].data_ptr()), dict(tptr=out["dc"].data_ptr()), dict(tptr=out["ac_exact"].data_ptr()),
            dict(tptr=idx.data_ptr()), dict(tptr=xd.data_ptr() + 64)]           # the records over an input
    if mode == H.QT:
        host.append(dict(qq=None))
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    # an index with one entry raised by one: a checked refusal on the device, and the next call succeeds
    ix = idx.clone()
    ix[2] += 1
    assert call(ixptr=ix.data_ptr()) == H.E_ARG
    after()
    assert info.cnt > 0
    assert call(cnt=info.cnt - 1) == H.E_ARG
    after()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_nan_block_stays_in_its_tile(ctx, dtype):
    """tests/nonfinite.py's qnan_one: one NaN in an interior block -- its DC and with it the whole block decode to NaN.  The
    tile's sums are NaN, its extremes pass the block over; every other tile's record is, byte for byte, that of the same array
    with the block finite (a NaN is passed over by the statistics: sf is the same)."""
    n, mode = FLAT_N[-1], H.EC
    base = _field(n, "noisy", dtype, seed=n) * dtype(0.09)          # |x| < 100, as nonfinite.make asks; sf = 10
    assert float(np.abs(base).max()) > 10.0
    x, bad = NF.make("qnan_one", n, dtype, base=base)
    assert bad.size == 1
    tile = int(bad[0]) // 64
    xd, out, info, full, idx, q = _streams(ctx, x, mode)
    bd, bout, binfo, bfull, bidx, bq = _streams(ctx, base, mode)
    assert info.sf == binfo.sf == 10.0
    lo = 64 * int(bad[0])
    assert np.isnan(full[lo:lo + 64]).all() and int(np.isnan(full).sum()) == 64
    want, mag, wt, mt = _reduce(full, x)
    for ref, bref in ((None, None), (xd, bd)):
        recs, total = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, ref=ref)
        brecs, _ = ctx.tile_summary(bout, binfo.cnt, n, _tdt(dtype), EB, binfo.sf, index=bidx, ref=bref)
        r, b = recs.cpu().numpy(), brecs.cpu().numpy()
        fs = [f for f in SUMS if ref is not None or f < 4]
        fe = [f for f in EXTREMES if ref is not None or f < 4]
        assert np.isnan(r[tile, fs]).all() and not np.isnan(r[tile, fe]).any()
        assert np.array_equal(_bits(r[tile, fe]), _bits(want[tile, fe]))
        others = np.arange(r.shape[0]) != tile
        assert np.array_equal(_bits(r[others]), _bits(b[others]))
        assert all(np.isnan(getattr(total, FIELDS[f])) for f in fs)
        assert np.array_equal(_bits(np.array([getattr(total, FIELDS[f]) for f in fe])), _bits(wt[fe]))


def test_all_nan_tile_reports_the_starting_pair(ctx):
    """A tile of nothing but NaNs: rmin = +DBL_MAX, rmax = -DBL_MAX (k_psnr's starting pair), emax = 0."""
    n, dtype = 3 * 4096, np.float64
    base = _field(n, "smooth", dtype, seed=1) * 0.09
    x, bad = NF.make("nan_tile", n, dtype, base=base)
    assert np.array_equal(bad, np.arange(64, 128))
    xd, out, info, full, idx, q = _streams(ctx, x, H.EC)
    assert np.isnan(full[4096:8192]).all()
    recs, total = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, ref=xd)
    r = recs.cpu().numpy()
    assert r[1, 0] == DBL_MAX and r[1, 1] == -DBL_MAX and r[1, 6] == 0.0 and np.isnan(r[1, [2, 3, 7]]).all()
    assert r[1, 4] == float(np.nanmin(x[4096:8192])) and r[1, 5] == float(np.nanmax(x[4096:8192]))
    assert total.rmin == min(r[0, 0], r[2, 0]) and total.rmax == max(r[0, 1], r[2, 1])


def test_tiles_worth_decoding(ctx):
    """The use case: the tiles whose record says rmax > thr are exactly the tiles where the full decode exceeds thr."""
    n, dtype, mode = FLAT_N[-1], np.float32, H.QT
    x, xd, out, info, full, idx, q, *_ = _data(ctx, n, dtype, mode, "noisy")
    recs, _ = ctx.tile_summary(out, info.cnt, n, _tdt(dtype), EB, info.sf, index=idx, mode=mode, qtable=q)
    r = recs.cpu().numpy()
    tiles = r.shape[0]
    tile_max = np.array([full[t * TILE:min(t * TILE + TILE, n)].max() for t in range(tiles)], dtype=np.float64)
    thr = float(np.sort(tile_max)[tiles // 2 - 1])        # the lower median: some tiles above, some not
    hit = np.flatnonzero(r[:, 1] > thr)
    want = np.flatnonzero(np.array([(full[t * TILE:min(t * TILE + TILE, n)] > thr).any() for t in range(tiles)]))
    assert 0 < hit.size < tiles and np.array_equal(hit, want)
