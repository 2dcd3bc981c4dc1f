"""Every flat entry point on an array past 4 GiB (tests/size_cases.py: workload F, 537 929 784 doubles = 4 303 438 272 bytes).

The array is a pattern of 257 tiles repeated 511 times plus a tail that ends in a short block; 2^32 bytes lie inside the last
period and are no whole number of periods, so an offset that wraps or sign-extends lands on other data.  The model [pattern |
tail] is held to the independent references -- the oracle for streams and decode, the numpy restatements for the index, the
records, the correction list, the mask and the fill -- and predicts every output of the big array bit for bit.  Everything of
the big array's size is compared on the device.  Inexact comparisons name the existing test whose rule they apply.

One workload is alive at a time: the module fixture is parametrised (EC, QT, holes) and drops its tensors on teardown."""
import ctypes as C
import math

import numpy as np
import pytest

from dctz_amd import hip as H
from oracle import oracle as O
from tests import mask_cases as M
from tests import size_cases as Z
from tests.test_gpu_rd_probe import EBS, SSE_RTOL_F64
from tests.test_gpu_tile_summary import _bound, _check, _reduce

pytestmark = pytest.mark.gpu

W = Z.F
EB = Z.EB
LINE = Z.FOUR_GIB // 8                                   # the first element past 4 GiB
FILL = -9.96921e36
FLAGS, VALUE, LIMIT = M.RULES[Z.HOLES[0]]
ROWS_2D = W.views[1][0]


def _np_u(t, dt):
    return t.cpu().numpy().view(dt)


class Big:
    """The model and the big array on the device with their streams, index and full decode (kind `ragged`), or with nothing
    but the arrays (kind `holes`: the mask tests make their own outputs)."""

    def __init__(self, ctx, kind, mode):
        import torch
        self.ctx, self.mode, self.tdt = ctx, mode, torch.float64
        self.p = Z.pattern(W, kind)
        self.s = Z.model(W, self.p)
        self.ns = self.s.size
        self.sd = torch.from_numpy(self.s).to(ctx.device)
        self.x = Z.expand(self.sd, W.reps, W.period)
        assert self.x.numel() == W.n and self.x.numel() * 8 > Z.FOUR_GIB
        if kind == "holes":
            return
        # the model against the oracle
        c = self.c = O.compress(self.s, EB, mode, O.FAST)
        self.outs, self.infos = ctx.compress(self.sd, EB, mode)
        assert (self.infos.sf, self.infos.cnt) == (c.sf, c.cnt) and c.sf == 10.0
        assert (self.infos.max_abs, self.infos.min_abs) == (c.stats.max, c.stats.min)
        assert np.array_equal(_np_u(self.outs["bin_index"], np.uint8), c.bin_index)
        assert np.array_equal(_np_u(self.outs["dc"], np.uint32), c.dc.view(np.uint32))
        assert np.array_equal(_np_u(self.outs["ac_exact"][:c.cnt], np.uint32), c.ac_exact.view(np.uint32))
        self.q = np.array(self.infos.qtable[:]) if mode == H.QT else None
        if mode == H.QT:
            assert np.array_equal(self.q.view(np.uint64), c.qtable.view(np.uint64))
        self.fulls = ctx.decompress(self.outs, c.cnt, self.ns, self.tdt, EB, c.sf, mode, qtable=self.q)
        self.fulls_np = self.fulls.cpu().numpy()
        assert np.array_equal(self.fulls_np.view(np.uint64), O.decompress(c, O.FAST).view(np.uint64))
        self.idxs, tot = ctx.ac_index(self.outs, self.ns)
        assert tot == c.cnt and np.array_equal(_np_u(self.idxs, np.uint32), Z.flat_index(c.bin_index))
        self.cp, self.ct = Z.period_counts(c.bin_index, W)
        assert self.cp > 0 and self.ct > 0
        # the big array: compressed once, decoded once, indexed once
        self.out, self.info = ctx.compress(self.x, EB, mode)
        self.full = ctx.decompress(self.out, self.info.cnt, W.n, self.tdt, EB, self.info.sf, mode, qtable=self.q)
        self.idx, self.idx_total = ctx.ac_index(self.out, W.n)

    def args(self, model=False):
        """(out, cnt, n, dtype, eb, sf) as the decode-side calls take them."""
        if model:
            return self.outs, self.infos.cnt, self.ns, self.tdt, EB, self.infos.sf
        return self.out, self.info.cnt, W.n, self.tdt, EB, self.info.sf

    def drop(self):
        self.__dict__.clear()


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(ctx, request):
    import torch
    kind, mode = {"EC": ("ragged", H.EC), "QT": ("ragged", H.QT), "holes": ("holes", H.EC)}[request.param]
    b = Big(ctx, kind, mode)
    yield b
    b.drop()
    torch.cuda.empty_cache()


STREAMS = pytest.mark.parametrize("big", ["EC", "QT"], indirect=True)
STREAMS_EC = pytest.mark.parametrize("big", ["EC"], indirect=True)
HOLES = pytest.mark.parametrize("big", ["holes"], indirect=True)


def test_workload():
    Z.check_workloads()
    assert W.n == 537929784 and (W.reps - 1) * W.period < LINE < W.reps * W.period


# ---- streams, decode, index ----------------------------------------------------------------------------------------------
@STREAMS
def test_streams_and_decode_are_the_models(big):
    b = big
    assert (b.info.sf, b.info.max_abs, b.info.min_abs) == (b.infos.sf, b.infos.max_abs, b.infos.min_abs)
    assert bytes(b.info.qtable) == bytes(b.infos.qtable) and b.info.nblk == -(-W.n // 64)
    assert Z.streams_ok(W, b.out, b.info.cnt, b.outs, b.infos.cnt)
    assert Z.decode_ok(W, b.full, b.fulls)                                        # ... which is the oracle's decode of the model


@STREAMS
def test_ac_index(big):
    b = big
    assert b.idx_total == b.info.cnt == W.reps * b.cp + b.ct
    assert Z.index_ok(W, b.idx, b.idxs, b.cp)


# ---- ranges and boxes: slices of the whole-array decode (itself periodic against the oracle's, above) --------------------------
# (lo, hi) in elements: in the first period; across the 4 GiB line; the tail with its short block; across several periods; and
# one longer than 2^29 elements, whose OUTPUT offsets pass 4 GiB as well
RANGES = [(100, 70001), (LINE - 70001, LINE + 70003), (W.n - 9001, W.n), (3 * W.period - 1000, 6 * W.period + 333),
          (W.period // 2 + 3, W.period // 2 + 3 + (1 << 29) + 4099)]


@STREAMS
def test_decompress_range(big):
    b = big
    assert RANGES[1][0] * 8 < Z.FOUR_GIB < RANGES[1][1] * 8 and RANGES[2][1] > W.n // 64 * 64 > RANGES[2][0]
    assert (RANGES[4][1] - RANGES[4][0]) * 8 > Z.FOUR_GIB
    for lo, hi in RANGES:
        r = b.ctx.decompress_range(*b.args(), lo, hi, b.idx, mode=b.mode, qtable=b.q)
        assert Z.same(r, b.full[lo:hi]), (lo, hi)
        del r


def _row_boxes(view):
    """Boxes of a view of F whose first axis has `rows` rows (the other axes are cut on both sides): in the first period,
    across the 4 GiB line, in the tail down to the last element (short block included), across several periods."""
    rows, rest = view[0], view[1:]
    per_row = W.n // rows
    line_row = LINE // per_row
    period_rows = W.period // per_row
    inner_lo = tuple(min(1, d - 1) for d in rest)
    inner_hi = tuple(max(l + 1, d - 1) for l, d in zip(inner_lo, rest))
    return [((3,) + inner_lo, (period_rows - 7,) + inner_hi),
            ((line_row - 20,) + inner_lo, (line_row + 21,) + inner_hi),
            ((rows - 4,) + (0,) * len(rest), (rows,) + tuple(rest)),
            ((2 * period_rows - 5,) + inner_lo, (5 * period_rows + 9,) + inner_hi)]


def _sl(lo, hi):
    return tuple(slice(l, h) for l, h in zip(lo, hi))


@STREAMS
def test_decompress_box(big):
    b = big
    for view in W.views[1:]:
        whole = b.full.view(view)
        for lo, hi in _row_boxes(view):
            r = b.ctx.decompress_box(b.out, b.info.cnt, view, b.tdt, EB, b.info.sf, lo, hi, b.idx, mode=b.mode, qtable=b.q)
            assert Z.same(r, whole[_sl(lo, hi)].contiguous()), (view, lo, hi)
            del r


@STREAMS
def test_decompress_boxes(big):
    """All four placements in one list, per view; the 1-D view takes the ranges (the longest left out: one list, one output each)."""
    b = big
    for view in W.views:
        boxes = [((lo,), (hi,)) for lo, hi in RANGES[:4]] if len(view) == 1 else _row_boxes(view)
        outs = b.ctx.decompress_boxes(b.out, b.info.cnt, view, b.tdt, EB, b.info.sf, boxes, b.idx, mode=b.mode, qtable=b.q)
        whole = b.full.view(view)
        for (lo, hi), r in zip(boxes, outs):
            assert Z.same(r, whole[_sl(lo, hi)].contiguous()), (view, lo, hi)
        del outs


# ---- tile summaries --------------------------------------------------------------------------------------------------------
@STREAMS
def test_tile_summary(big):
    """Records periodic against the model's, which test_gpu_tile_summary's _check holds to the numpy reductions.  The total:
    extremes are those of the device's records (and the model's); a sum is held against math.fsum of the device's records
    with test_gpu_tile_summary's bound for any order of summation, here of one term per tile."""
    import torch
    b = big
    want = _reduce(b.fulls_np, b.s)
    for ref_s, ref_b in ((None, None), (b.sd, b.x)):
        what = f"F ref={ref_b is not None}"
        recs_s, total_s = b.ctx.tile_summary(*b.args(model=True), index=b.idxs, mode=b.mode, qtable=b.q, ref=ref_s)
        _check(recs_s.cpu().numpy(), total_s, *want, b.ns, ref_s is not None, "model of " + what)
        recs, total = b.ctx.tile_summary(*b.args(), index=b.idx, mode=b.mode, qtable=b.q, ref=ref_b)
        assert Z.records_ok(W, recs, recs_s), what
        host = recs.cpu().numpy()
        assert host.shape == (W.tiles, 8)
        for f, name in enumerate(H.TileSummary._fields_):
            got, got_s = getattr(total, name[0]), getattr(total_s, name[0])
            if ref_b is None and f >= 4:
                assert got == 0.0, (what, name[0])
            elif f in (0, 4):
                assert got == float(torch.min(recs[:, f]).item()) == got_s, (what, name[0])
            elif f in (1, 5, 6):
                assert got == float(torch.max(recs[:, f]).item()) == got_s, (what, name[0])
            else:
                exact = math.fsum(host[:, f].tolist())
                bound = _bound(W.tiles, math.fsum(np.abs(host[:, f]).tolist()))
                print(f"{what}: total {name[0]} = {got!r}, fsum of the records = {exact!r}, bound = {bound:.3g}")
                assert abs(got - exact) <= bound, (what, name[0], got, exact, bound)
        if ref_b is not None:
            # dctzhip_psnr_terms on the same pair: extremes exact, the sum within the bound of n terms
            # (test_gpu_tile_summary.py::test_records_are_the_reductions_of_the_full_decode)
            pt = b.ctx.psnr_terms(b.x, b.full)
            assert (pt[0], pt[1], pt[2]) == (total.xmin, total.xmax, total.emax), (pt, what)
            esq = math.fsum(host[:, 7].tolist())
            assert abs(pt[3] - esq) <= _bound(W.n, esq), (pt[3], esq)
            assert abs(total.esq - pt[3]) <= _bound(W.n, esq), (total.esq, pt[3])


@STREAMS_EC
def test_stats(big):
    """dctzhip_stats: max |x|, min |x| and sf exact; the mean to test_gpu_parity's rule for another order of summation."""
    b = big
    st = H.CompressInfo()
    b.ctx._bind_stream()
    assert b.ctx.lib.dctzhip_stats(b.ctx.h, b.x.data_ptr(), W.n, H.F64, C.byref(st)) == 0
    assert (st.max_abs, st.min_abs, st.sf) == (b.c.stats.max, b.c.stats.min, b.c.sf)
    mean = (W.reps * math.fsum(b.p.tolist()) + math.fsum(b.s[W.period:].tolist())) / W.n
    assert abs(st.mean - mean) <= 1e-5 * max(1.0, abs(mean)), (st.mean, mean)
    assert abs(b.info.mean - mean) <= 1e-5 * max(1.0, abs(mean)), (b.info.mean, mean)


# ---- the correction list -----------------------------------------------------------------------------------------------------
@STREAMS
def test_fixup_build_and_apply(big):
    import torch
    b = big
    bound = EB * b.info.sf
    fix_s = b.ctx.fixup_build(*b.args(model=True), b.sd, bound, index=b.idxs, mode=b.mode, qtable=b.q)
    ws, wo, wv, wk = Z.flat_fix_list(b.s, b.fulls_np, bound)
    assert fix_s[3] == wk > 0 and np.array_equal(_np_u(fix_s[0], np.uint32), ws)
    assert np.array_equal(_np_u(fix_s[1], np.uint16), wo) and np.array_equal(_np_u(fix_s[2], np.uint64), wv.view(np.uint64))
    count_only = b.ctx.fixup_build(*b.args(), b.x, bound, index=b.idx, mode=b.mode, qtable=b.q, capacity=0)
    assert Z.fix_ok(W, count_only, fix_s)
    fix = b.ctx.fixup_build(*b.args(), b.x, bound, index=b.idx, mode=b.mode, qtable=b.q, capacity=count_only[3])
    assert Z.fix_ok(W, fix, fix_s) and Z.same(fix[0], count_only[0])
    # apply to the whole decode: afterwards !(|x - r| <= bound) holds nowhere (independent of the model) ...
    applied_s = b.ctx.fixup_apply(fix_s, b.ns, b.tdt, b.fulls.clone())
    with np.errstate(invalid="ignore"):
        listed = ~(np.abs(b.s - b.fulls_np) <= bound)
    assert np.array_equal(applied_s.cpu().numpy().view(np.uint64), np.where(listed, b.s, b.fulls_np).view(np.uint64))
    applied = b.ctx.fixup_apply(fix, W.n, b.tdt, b.full.clone())
    assert not bool((~((b.x - applied).abs() <= bound)).any().item())
    assert Z.decode_ok(W, applied, applied_s)                                     # ... and nothing else was touched
    # ... and to a box across the 4 GiB line
    view = W.views[1]
    lo, hi = _row_boxes(view)[1]
    box = b.ctx.decompress_box(b.out, b.info.cnt, view, b.tdt, EB, b.info.sf, lo, hi, b.idx, mode=b.mode, qtable=b.q)
    b.ctx.fixup_apply(fix, W.n, b.tdt, box.view(-1), dims=view, lo=lo, hi=hi)
    assert Z.same(box, applied.view(view)[_sl(lo, hi)].contiguous())
    assert not Z.same(box, b.full.view(view)[_sl(lo, hi)].contiguous())           # the box holds corrected elements


# ---- the rate-distortion probe -------------------------------------------------------------------------------------------------
@STREAMS_EC
def test_rd_probe(big):
    """16 bounds: every count is reps * cnt_P + cnt_tail exactly, cnt_P and cnt_tail from probing P alone and the model (both
    held to the oracle's counts); the predicted SSE against the same combination within test_gpu_rd_probe's SSE_RTOL_F64."""
    import torch
    b = big
    pp, rng_p = b.ctx.rd_probe(torch.from_numpy(b.p).to(b.ctx.device), EBS)
    ps, rng_s = b.ctx.rd_probe(b.sd, EBS)
    for eb, a, s in zip(EBS, pp, ps):
        c = O.compress(b.s, eb, H.EC, O.FAST)
        assert (a["cnt"], s["cnt"] - a["cnt"]) == Z.period_counts(c.bin_index, W) and s["cnt"] == c.cnt, eb
    pb, rng_b = b.ctx.rd_probe(b.x, EBS)
    assert rng_b == rng_s == rng_p == (float(b.s.min()), float(b.s.max()))
    assert Z.probe_ok(W, [v["cnt"] for v in pb], [v["cnt"] for v in pp], [v["cnt"] for v in ps])
    assert pb[EBS.index(EB)]["cnt"] == b.info.cnt
    want = Z.probe_counts(W, [v["sse"] for v in pp], [v["sse"] for v in ps])
    for eb, v, sse in zip(EBS, pb, want):
        assert v["error_bound"] == eb and v["raw_bytes"] == W.n + 4 * (-(-W.n // 64)) + 4 * v["cnt"] + 56
        assert abs(v["sse"] - sse) <= SSE_RTOL_F64 * sse, (eb, v["sse"], sse)


# ---- missing values ----------------------------------------------------------------------------------------------------------
@HOLES
def test_mask_build_apply_and_compress_masked(big):
    """The pattern carries mask_cases' blobs of 1e36, -1e33, Inf and NaN markers and the special values that stay valid.
    Words, filled copy and count are predicted from the model, which is held to mask_cases' numpy fill."""
    import torch
    b, ctx = big, big.ctx
    miss_s = M.is_missing(b.s, FLAGS, VALUE, LIMIT)
    want_f = M.fill(b.s, miss_s)
    mask_s, count_s, filled_s = ctx.mask_build(b.sd, FLAGS, VALUE, LIMIT)
    assert count_s == int(miss_s.sum()) > 0 and np.array_equal(_np_u(mask_s, np.uint64), M.mask_words(miss_s))
    assert np.array_equal(_np_u(filled_s, np.uint64), want_f.view(np.uint64))
    # out of place, in place, mask only
    mask, count, filled = ctx.mask_build(b.x, FLAGS, VALUE, LIMIT)
    assert Z.mask_ok(W, mask, count, mask_s, count_s) and Z.decode_ok(W, filled, filled_s)
    miss = torch.isnan(b.x) | (b.x.abs() >= LIMIT)                                # (Inf included; independent of the model)
    assert count == int(miss.sum().item())
    x2 = b.x.clone()
    mask2, count2, f2 = ctx.mask_build(x2, FLAGS, VALUE, LIMIT, filled=x2)
    assert count2 == count and Z.same(mask2, mask) and Z.same(x2, filled)
    del x2, f2
    mask3, count3, f3 = ctx.mask_build(b.x, FLAGS, VALUE, LIMIT, filled=False)
    assert f3 is None and count3 == count and Z.same(mask3, mask)
    # apply: the whole array, and a box across the 4 GiB line
    whole = ctx.mask_apply(mask, W.n, FILL, filled.clone())
    assert Z.same(whole, torch.where(miss, torch.full_like(filled, FILL), filled))
    view = W.views[1]
    lo, hi = _row_boxes(view)[1]
    box = filled.view(view)[_sl(lo, hi)].contiguous()
    ctx.mask_apply(mask, W.n, FILL, box.view(-1), dims=view, lo=lo, hi=hi)
    assert Z.same(box, whole.view(view)[_sl(lo, hi)].contiguous()) and bool((box == FILL).any().item())
    del whole, miss
    # compress_masked: the mask, the filled copy, and the streams of the filled array
    c = O.compress(want_f, EB, H.EC, O.FAST)
    fs = torch.empty_like(b.sd)
    outs, infos, ms, ks = ctx.compress_masked(b.sd, EB, FLAGS, VALUE, LIMIT, filled=fs)
    assert (infos.sf, infos.cnt, ks) == (c.sf, c.cnt, count_s) and Z.same(ms, mask_s) and Z.same(fs, filled_s)
    assert np.array_equal(_np_u(outs["bin_index"], np.uint8), c.bin_index)
    assert np.array_equal(_np_u(outs["dc"], np.uint32), c.dc.view(np.uint32))
    assert np.array_equal(_np_u(outs["ac_exact"][:c.cnt], np.uint32), c.ac_exact.view(np.uint32))
    fb = torch.empty_like(b.x)
    out, info, mb, kb = ctx.compress_masked(b.x, EB, FLAGS, VALUE, LIMIT, filled=fb)
    assert (info.sf, info.max_abs, info.min_abs) == (infos.sf, infos.max_abs, infos.min_abs) and kb == count
    assert Z.same(mb, mask) and Z.same(fb, filled)
    assert Z.streams_ok(W, out, info.cnt, outs, infos.cnt)
