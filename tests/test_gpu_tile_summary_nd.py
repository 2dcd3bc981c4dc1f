"""Tile summaries of arrays compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h: dctzhip_tile_summary_nd): one record per
stream tile of what dctzhip_decompress_nd writes -- min, max, sum, sum of squares over the array's own elements -- and, with
the original read in place, min / max of the original, max |x - r| and sum (x - r)^2, without the reconstruction being written.

Reference: the library's own ctx.decompress_nd of the same streams (code from before this layer), reduced per stream tile over
the real positions in numpy (tests/ndsummary_cases.py).
  * extremes are equal as bits; e = x - r is formed in the array's dtype;
  * a sum over m terms lies within (m - 1) u / (1 - (m - 1) u) sum |t_i| of math.fsum, u = 2^-53, m the tile's real positions:
    the bound for ANY order of summation, not a measured number.  compress_nd pads an edge tile by repeating samples, so a
    padded position decodes to a value near 100: one of them counted moves rsum by about 100 against a bound near 2e-7.
"""
import ctypes as C
import math

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import ndsummary_cases as S

pytestmark = pytest.mark.gpu

EB = S.EB
FIELDS, EXTREMES, SUMS = S.FIELDS, S.EXTREMES, S.SUMS
CASES = [(s, dt, mode, kind) for s in S.SHAPES for dt in (np.float64, np.float32) for mode in (H.EC, H.QT) for kind in S.KINDS]
RAGGED = [(45, 77), (13, 22, 35)]
MULTI = [(45, 200), (13, 22, 35)]     # ragged, and more than one stream tile (3 and 4)
GUARD = 63                            # band elements around an original read in place: the slice is aligned to its elements only


def _id(c):
    s, dt, mode, kind = c
    return f"{kind}-{'x'.join(map(str, s))}-{np.dtype(dt).name}-{'QT' if mode == H.QT else 'EC'}"


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Streams:
    """One array on the device with its streams, index, table, full decode and the reference reduction of that decode."""

    def __init__(self, ctx, x, mode):
        import torch
        self.x, self.shape, self.mode, self.dtype = x, tuple(x.shape), mode, x.dtype.type
        self.tdt = _tdt(x.dtype)
        self.xd = torch.from_numpy(x).to(ctx.device)
        self.out, self.info = ctx.compress_nd(self.xd, EB, mode)
        self.q = np.array(self.info.qtable[:]) if mode == H.QT else None
        self.sf, self.cnt = self.info.sf, self.info.cnt
        self.full_d = ctx.decompress_nd(self.out, self.cnt, self.shape, self.tdt, EB, self.sf, mode, qtable=self.q)
        self.full = self.full_d.cpu().numpy()
        self.n_lin = 64 * S.nblk(self.shape)
        self.idx, tot = ctx.ac_index(self.out, self.n_lin)
        assert tot == self.cnt
        self.want, self.mag, self.m, self.wt, self.mt = S.reduce(self.shape, self.full, x)

    def summary(self, ctx, ref, index="own", c=None):
        return (c or ctx).tile_summary_nd(self.out, self.cnt, self.shape, self.tdt, EB, self.sf, index=self.idx if index == "own" else index,
                                          mode=self.mode, qtable=self.q, ref=ref)

    def raw(self, ctx, tiles_ptr, total_ref, ref="own", **kw):
        q = np.ascontiguousarray(self.q, dtype=self.dtype) if self.q is not None else None
        a = dict(bin=self.out["bin_index"].data_ptr(), dc=self.out["dc"].data_ptr(), ac=self.out["ac_exact"].data_ptr(), idx=self.idx.data_ptr(),
                 dims=self.shape, cnt=self.cnt, q=q, mode=self.mode)
        a.update(kw)
        dims = None if a["dims"] is None else (C.c_size_t * len(a["dims"]))(*a["dims"])
        refp = self.xd.data_ptr() if isinstance(ref, str) else ref
        return ctx.lib.dctzhip_tile_summary_nd(
            ctx.h, a["bin"], a["dc"], a["ac"], int(a["cnt"]), a["idx"], a["q"].ctypes.data_as(C.c_void_p) if a["q"] is not None else None,
            0 if dims is None else len(a["dims"]), dims, H._dt(self.tdt), EB, float(self.sf), a["mode"], refp, tiles_ptr, total_ref)

    def flag_fraction(self):
        b = self.out["bin_index"].cpu().numpy()[:self.n_lin].reshape(-1, 64)[:, 1:]
        return float((b == 255).mean())


_DATA = {}


def _data(ctx, shape, dtype, mode, kind):
    key = (shape, np.dtype(dtype).name, mode, kind)
    if key not in _DATA:
        _DATA[key] = Streams(ctx, S.field(shape, kind, dtype), mode)
    return _DATA[key]


def _check(recs, total, s, with_ref, what):
    """recs (tiles, 8) numpy and total (a TileSummary) against the reduction of the full decode."""
    nt = S.tiles(s.shape)
    n = int(np.prod(s.shape))
    assert recs.shape == (nt, 8), what
    tot = np.array([getattr(total, f) for f in FIELDS])
    if not with_ref:
        assert not _bits(recs[:, 4:]).any() and not _bits(tot[4:]).any(), what        # +0.0 in all four
    fields_e = [f for f in EXTREMES if with_ref or f < 4]
    fields_s = [f for f in SUMS if with_ref or f < 4]
    for f in fields_e:
        assert np.array_equal(_bits(recs[:, f]), _bits(s.want[:, f])), (what, FIELDS[f])
    worst = 0.0
    for t in range(nt):
        for f in fields_s:
            b = S.bound(int(s.m[t]), s.mag[t, f])
            err = abs(recs[t, f] - s.want[t, f])
            worst = max(worst, err / b if b else (0.0 if err == 0 else math.inf))
            assert err <= b, (what, t, FIELDS[f], recs[t, f], s.want[t, f], b)
    print(f"{what}: worst |sum - fsum| / bound over the records = {worst:.3g}")
    for f in fields_e:
        pick = np.min if f in (0, 4) else np.max
        assert _bits(tot[f:f + 1])[0] == _bits(np.array([pick(recs[:, f])]))[0], (what, FIELDS[f])
        assert _bits(tot[f:f + 1])[0] == _bits(s.wt[f:f + 1])[0], (what, FIELDS[f])
    for f in fields_s:
        b = S.bound(n, s.mt[f])
        print(f"{what}: total {FIELDS[f]} = {tot[f]!r}, fsum = {s.wt[f]!r}, bound = {b:.3g}")
        assert abs(tot[f] - s.wt[f]) <= b, (what, FIELDS[f], tot[f], s.wt[f], b)


def _kernel_name(s, ref):
    return f"k_ndsummary<{'double' if s.dtype == np.float64 else 'float'}, {s.mode}, {len(s.shape) - 1}, {'true' if ref else 'false'}>"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_records_are_the_reductions_of_the_full_decode(ctx, case):
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    assert s.sf == 100.0                                  # the de-scale multiply runs
    assert (s.m >= 1).all() and int(s.m.sum()) == int(np.prod(shape))
    if S.nblk(shape) >= 64:
        # noisy fields store about three coefficients in ten exactly, at every position.  A smooth field is smooth along the
        # flattened index, so across the rows of a tile it is a ramp: a few low coefficients per block are stored exactly
        # (the flat test's "none" does not carry over), far fewer than with noise.
        p = s.flag_fraction()
        print(f"{_id(case)}: exactly stored fraction = {p:.4f}")
        assert (0.2 < p < 0.45) if kind == "noisy" else p < 0.1, p
    if shape in RAGGED:
        # the padding decodes to repeated samples near 100: counted, it would move rsum by more than any bound here
        pad = ~S.real(shape)
        assert pad.any() and S.bound(int(s.m.max()), s.mag[:, 2].max()) < 1e-6 and float(s.full.min()) > 1.0
    for ref in (None, s.xd):
        what = f"{_id(case)} ref={ref is not None}"
        recs, total = s.summary(ctx, ref)
        assert ctx.last_kernel(1) == _kernel_name(s, ref is not None)
        r1 = recs.cpu().numpy()
        _check(r1, total, s, ref is not None, what)
        # the same call twice: the same bytes in every record and in the total; index=None builds the index itself
        recs2, total2 = s.summary(ctx, ref, index=None)
        assert np.array_equal(_bits(recs2.cpu().numpy()), _bits(r1)), what
        assert bytes(total2) == bytes(total), what


@pytest.mark.parametrize("case", [(sh, dt, H.EC, "noisy") for sh in S.SHAPES for dt in (np.float64, np.float32)], ids=_id)
def test_total_agrees_with_psnr_terms(ctx, case):
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    n = int(np.prod(shape))
    _, total = s.summary(ctx, s.xd)
    pt = np.array(ctx.psnr_terms(s.xd.view(-1), s.full_d.view(-1)))
    got = np.array([total.xmin, total.xmax, total.emax])
    assert np.array_equal(_bits(got), _bits(pt[:3])), (got, pt)
    assert abs(total.esq - pt[3]) <= S.bound(n, s.mt[7]), (total.esq, pt[3])
    want = 20.0 * np.log10((pt[1] - pt[0]) / np.sqrt(pt[3] / n))
    assert abs(total.psnr(n) - want) <= 1e-9 * abs(want), (total.psnr(n), want)


@pytest.mark.parametrize("fill", [float("nan"), -7.25e11], ids=["nan", "sentinel"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda v: "x".join(map(str, v)))
def test_the_original_is_read_in_place_only(ctx, shape, dtype, fill):
    """The original as a contiguous slice of a larger buffer filled with NaN (then with a huge finite value, which extremes would
    not pass over), 63 elements from its start: the same bytes as with the original alone."""
    import torch
    s = _data(ctx, shape, dtype, H.EC, "noisy")
    good, good_total = s.summary(ctx, s.xd)
    buf = torch.full((s.x.size + 2 * GUARD,), fill, dtype=s.tdt, device=ctx.device)
    mid = buf[GUARD:GUARD + s.x.size].view(s.shape)
    mid.copy_(s.xd)
    assert mid.data_ptr() % 16 != 0 and mid.is_contiguous()
    recs, total = s.summary(ctx, mid)
    assert np.array_equal(_bits(recs.cpu().numpy()), _bits(good.cpu().numpy()))
    assert bytes(total) == bytes(good_total)


@pytest.mark.parametrize("case", [((13, 22, 35), np.float64, H.EC, "noisy"), ((45, 200), np.float32, H.QT, "noisy")], ids=_id)
def test_a_second_context_gives_the_same_bytes(ctx, case):
    import dctz_amd
    s = _data(ctx, *case)
    other = dctz_amd.Context(0)
    try:
        for ref in (None, s.xd):
            a, ta = s.summary(ctx, ref)
            b, tb = s.summary(ctx, ref, c=other)
            a2, ta2 = s.summary(ctx, ref)
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())) and bytes(ta) == bytes(tb)
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(a2.cpu().numpy())) and bytes(ta) == bytes(ta2)
    finally:
        other.close()


def test_more_tiles_than_resident_workgroups(ctx):
    """2560 stream tiles: a workgroup takes several (the grid-stride loop) and k_tile_summary_final runs two levels."""
    s = Streams(ctx, S.field(S.BIG, "noisy", np.float64), H.EC)
    assert S.tiles(S.BIG) == 2560
    recs, total = s.summary(ctx, s.xd)
    _check(recs.cpu().numpy(), total, s, True, "big ref=True")


def test_total_alone_and_records_alone(ctx):
    """d_tiles == NULL keeps the records in scratch of the context; total == NULL joins nothing."""
    import torch
    s = _data(ctx, (13, 22, 35), np.float64, H.EC, "noisy")
    for ref in (None, s.xd):
        recs, total = s.summary(ctx, ref)
        refp = None if ref is None else ref.data_ptr()
        t2 = H.TileSummary()
        assert s.raw(ctx, None, C.byref(t2), ref=refp) == H.OK and bytes(t2) == bytes(total)
        r2 = torch.zeros_like(recs)
        assert s.raw(ctx, r2.data_ptr(), None, ref=refp) == H.OK
        assert np.array_equal(_bits(r2.cpu().numpy()), _bits(recs.cpu().numpy()))
        assert s.raw(ctx, None, None, ref=refp) == H.E_ARG


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("shape", MULTI, ids=lambda v: "x".join(map(str, v)))
def test_refusals_leave_the_context_usable(ctx, shape, dtype, mode):
    import torch
    s = _data(ctx, shape, dtype, mode, "noisy")
    es = np.dtype(dtype).itemsize
    good, good_total = s.summary(ctx, s.xd)
    recs = torch.zeros_like(good)
    total = H.TileSummary()

    def call(tptr=None, ref="own", **kw):
        return s.raw(ctx, recs.data_ptr() if tptr is None else tptr, C.byref(total), ref=ref, **kw)

    def after():
        assert call() == H.OK
        assert np.array_equal(_bits(recs.cpu().numpy()), _bits(good.cpu().numpy())) and bytes(total) == bytes(good_total)

    after()
    host = [dict(dims=shape[:1]), dict(dims=(8, 8, 8, 8)), dict(dims=None),                        # ndims not 2 or 3, no extents
            dict(dims=shape[:-1] + (0,)), dict(dims=(0,) + shape[1:]),                             # a zero extent
            dict(bin=0), dict(bin=s.out["bin_index"].data_ptr() + 4), dict(dc=0), dict(dc=s.out["dc"].data_ptr() + 2),
            dict(idx=0), dict(idx=s.idx.data_ptr() + 2), dict(ac=0), dict(ac=s.out["ac_exact"].data_ptr() + 2),
            dict(ref=s.xd.data_ptr() + es // 2),                                                   # the original not aligned to its elements
            dict(tptr=recs.data_ptr() + 4),                                                        # the records not 8-byte aligned
            dict(tptr=s.out["bin_index"].data_ptr()), dict(tptr=s.out["dc"].data_ptr()), dict(tptr=s.out["ac_exact"].data_ptr()),
            dict(tptr=s.idx.data_ptr()), dict(tptr=s.xd.data_ptr() + 64)]                          # the records over an input
    if mode == H.QT:
        host.append(dict(q=None))
    for kw in host:
        assert call(**kw) == H.E_ARG, kw
        after()
    assert s.raw(ctx, None, None) == H.E_ARG                                                      # nothing asked for
    after()
    # checked refusals on the device, each followed by a good call on the same context: an index with one entry raised by one;
    # an index built for another length (one tile fewer; its missing entry reads as zero); AC_exact one word short
    assert S.tiles(shape) >= 3 and s.cnt > 0
    ix = s.idx.clone()
    ix[2] += 1
    assert call(idx=ix.data_ptr()) == H.E_ARG
    after()
    short, _ = ctx.ac_index(s.out, s.n_lin - S.TILE)
    assert short.numel() < s.idx.numel()
    ix = torch.zeros_like(s.idx)
    ix[:short.numel()] = short
    assert call(idx=ix.data_ptr()) == H.E_ARG
    after()
    assert call(cnt=s.cnt - 1) == H.E_ARG
    after()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", MULTI, ids=lambda v: "x".join(map(str, v)))
def test_a_nan_block_stays_in_its_tile(ctx, shape, dtype):
    """One NaN in the original: its block's DC and with it the whole block decode to NaN.  The tile's sums are NaN, its extremes
    pass the block over; every other tile's record is, byte for byte, that of the same array with the block finite (the
    statistics pass a NaN over: sf is the same)."""
    base = S.field(shape, "noisy", dtype) * dtype(0.09)   # sf = 10
    assert 10.0 < float(np.abs(base).max()) < 100.0
    at = tuple(d - 2 for d in shape)                      # in the grid's last block, ragged on every axis
    x = base.copy()
    x[at] = np.nan
    tile = int(S.position(shape, at)) // S.TILE
    assert 0 < tile < S.tiles(shape)
    s, b = Streams(ctx, x, H.EC), Streams(ctx, base, H.EC)
    assert s.sf == b.sf == 10.0
    nan_at = S.to_stream(shape, np.isnan(s.full), False)
    assert nan_at.any() and set(np.flatnonzero(nan_at) >> 6) == {int(S.position(shape, at)) >> 6}      # the block, and nothing else
    for ref, bref in ((None, None), (s.xd, b.xd)):
        recs, total = s.summary(ctx, ref)
        brecs, _ = b.summary(ctx, bref)
        r, g = recs.cpu().numpy(), brecs.cpu().numpy()
        fs = [f for f in SUMS if ref is not None or f < 4]
        fe = [f for f in EXTREMES if ref is not None or f < 4]
        assert np.isnan(r[tile, fs]).all() and not np.isnan(r[tile, fe]).any()
        assert np.array_equal(_bits(r[tile, fe]), _bits(s.want[tile, fe]))
        others = np.arange(r.shape[0]) != tile
        assert np.array_equal(_bits(r[others]), _bits(g[others]))
        assert all(np.isnan(getattr(total, FIELDS[f])) for f in fs)
        assert np.array_equal(_bits(np.array([getattr(total, FIELDS[f]) for f in fe])), _bits(s.wt[fe]))
