"""Arrays compressed in 8 x 8 / 4 x 4 x 4 tiles at the size edges of their address arithmetic (tests/size_cases.py).

A2, A3 (3.2 GB, aligned): inside the window in which k_compress / k_decompress address the array in place through one buffer
descriptor, and past 2 GiB -- the descriptor's byte count and the byte offsets are negative as ints there.  G3a: aligned, just
past the window, so the threshold itself sends it to the gather / scatter passes.  G2, G3 (4.3 GB, ragged on every axis): past
2^32 bytes, every call family through its _nd twin.

The method is the flat file's: the model [pattern | tail rows] is held to the oracle and to the numpy restatements, and
predicts every output of the big array bit for bit; big data is compared on the device.  One workload is alive at a time."""
import math
import os
import types

import numpy as np
import pytest

from dctz_amd import hip as H
from oracle import oracle as O
from tests import mask_cases as M
from tests import ndfix_cases as NF
from tests import ndmask_cases as NM
from tests import ndsummary_cases as NS
from tests import size_cases as Z
from tests.rd_nd_cases import EBS, SSE_RTOL_F64
from tests.test_gpu_tile_summary_nd import _check as _check_records

pytestmark = pytest.mark.gpu

EB = Z.EB
LINE = Z.FOUR_GIB // 8                                   # the first element past 4 GiB
FLAGS, VALUE, LIMIT = M.RULES[Z.HOLES[0]]
WORKLOADS = {w.name: w for w in (Z.A2, Z.A3, Z.G2, Z.G3, Z.G3A)}
PROBE_ORACLE = EBS                                       # the bounds at which the model's counts are held to the oracle's


def _np_u(t, dt):
    return t.cpu().numpy().reshape(-1).view(dt)


class Big:
    """The model and the big array of workload w on the device, with their streams, index and full decode (kind `ragged`) or
    with nothing but the arrays (kind `holes`)."""

    def __init__(self, ctx, w, kind, mode):
        import torch
        self.ctx, self.w, self.mode, self.tdt = ctx, w, mode, torch.float64
        self.p = Z.pattern(w, kind)
        self.s = Z.model(w, self.p)
        self.sd = torch.from_numpy(self.s).to(ctx.device)
        self.x = Z.expand(self.sd, w.reps, w.period)
        assert tuple(self.x.shape) == w.shape and ctx.nd_blocks(w.shape) * 64 == w.stream_n
        assert ctx.nd_blocks(w.model_shape) * 64 == w.model_stream_n
        if kind == "holes":
            return
        # the model against the oracle
        c = self.c = O.compress_nd(self.s, EB, mode, O.FAST)
        self.outs, self.infos = ctx.compress_nd(self.sd, EB, mode)
        assert (self.infos.sf, self.infos.cnt) == (c.sf, c.cnt) and c.sf == 10.0
        assert (self.infos.max_abs, self.infos.min_abs) == (c.stats.max, c.stats.min)
        assert np.array_equal(_np_u(self.outs["bin_index"], np.uint8), c.bin_index)
        assert np.array_equal(_np_u(self.outs["dc"], np.uint32), c.dc.view(np.uint32))
        assert np.array_equal(_np_u(self.outs["ac_exact"][:c.cnt], np.uint32), c.ac_exact.view(np.uint32))
        self.q = np.array(self.infos.qtable[:]) if mode == H.QT else None
        if mode == H.QT:
            assert np.array_equal(self.q.view(np.uint64), c.qtable.view(np.uint64))
        self.fulls = ctx.decompress_nd(self.outs, c.cnt, w.model_shape, self.tdt, EB, c.sf, mode, qtable=self.q)
        self.fulls_np = self.fulls.cpu().numpy()
        assert np.array_equal(self.fulls_np.view(np.uint64), O.decompress_nd(c, w.model_shape, O.FAST).view(np.uint64))
        self.idxs, tot = ctx.ac_index(self.outs, w.model_stream_n)
        assert tot == c.cnt and np.array_equal(_np_u(self.idxs, np.uint32), Z.flat_index(c.bin_index))
        self.cp, self.ct = Z.period_counts(c.bin_index, w)
        assert self.cp > 0
        # the big array: compressed once, decoded once, indexed once
        self.out, self.info = ctx.compress_nd(self.x, EB, mode)
        self.full = ctx.decompress_nd(self.out, self.info.cnt, w.shape, self.tdt, EB, self.info.sf, mode, qtable=self.q)
        self.idx, self.idx_total = ctx.ac_index(self.out, w.stream_n)

    def args(self, model=False):
        """(out, cnt, shape, dtype, eb, sf) as the decode-side calls take them."""
        if model:
            return self.outs, self.infos.cnt, self.w.model_shape, self.tdt, EB, self.infos.sf
        return self.out, self.info.cnt, self.w.shape, self.tdt, EB, self.info.sf

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
    name, what = request.param.split("-")
    kind, mode = {"EC": ("ragged", H.EC), "QT": ("ragged", H.QT), "holes": ("holes", H.EC)}[what]
    b = Big(ctx, WORKLOADS[name], kind, mode)
    yield b
    b.drop()
    torch.cuda.empty_cache()


def _on(*names):
    return pytest.mark.parametrize("big", list(names), indirect=True)


def test_workloads():
    Z.check_workloads()


def _streams_and_decode(b):
    w = b.w
    assert (b.info.sf, b.info.max_abs, b.info.min_abs) == (b.infos.sf, b.infos.max_abs, b.infos.min_abs)
    assert bytes(b.info.qtable) == bytes(b.infos.qtable) and b.info.nblk == w.stream_n // 64
    assert b.info.cnt == w.reps * b.cp + b.ct
    assert Z.streams_ok(w, b.out, b.info.cnt, b.outs, b.infos.cnt)
    assert Z.decode_ok(w, b.full, b.fulls)
    assert b.idx_total == b.info.cnt and Z.index_ok(w, b.idx, b.idxs, b.cp)


# ---- the in-place window ---------------------------------------------------------------------------------------------------------
@_on("A2-EC", "A2-QT", "A3-EC", "A3-QT")
def test_in_place_window_past_2_gib(big):
    """compress_nd / decompress_nd read and write the array in place: streams and decode are the model's, extended; a context
    with DCTZHIP_ND_DIRECT=0 (the gather / scatter passes) gives the same bytes."""
    import dctz_amd
    b, w = big, big.w
    assert (1 << 31) < w.bytes <= Z.ND_WINDOW and w.tail == 0
    _streams_and_decode(b)
    if os.environ.get("DCTZHIP_SPECULATE", "1") != "0" and os.environ.get("DCTZHIP_ND_DIRECT", "1") != "0":
        assert b.info.flags & H.INFO_STATS_FUSED      # (tests/test_nd_blocks.py: the in-place call speculates, the gather path cannot)
    os.environ["DCTZHIP_ND_DIRECT"] = "0"
    try:
        cx = dctz_amd.Context(0)
    finally:
        os.environ.pop("DCTZHIP_ND_DIRECT", None)
    try:
        out, info = cx.compress_nd(b.x, EB, b.mode)
        assert not (info.flags & H.INFO_STATS_FUSED)
        assert (info.sf, info.cnt, info.max_abs, info.min_abs) == (b.info.sf, b.info.cnt, b.info.max_abs, b.info.min_abs)
        assert bytes(info.qtable) == bytes(b.info.qtable)
        assert Z.same(out["bin_index"], b.out["bin_index"]) and Z.same(out["dc"], b.out["dc"])
        assert Z.same(out["ac_exact"][:info.cnt], b.out["ac_exact"][:info.cnt])
        r = cx.decompress_nd(out, info.cnt, w.shape, b.tdt, EB, info.sf, b.mode, qtable=b.q)
        assert Z.same(r, b.full)
        del out, r
    finally:
        cx.close()


@_on("G3a-EC", "G3a-QT")
def test_aligned_array_just_past_the_window(big):
    """No tile is padded, yet one 32-bit descriptor no longer covers the array: the threshold sends it to gather / scatter."""
    b, w = big, big.w
    assert w.bytes > Z.ND_WINDOW and all(d % 4 == 0 for d in w.shape)
    _streams_and_decode(b)
    assert not (b.info.flags & H.INFO_STATS_FUSED)    # the in-place call's flag (test_in_place_window_past_2_gib)


# ---- past 2^32 bytes, ragged ---------------------------------------------------------------------------------------------------------
RAGGED = ("G2-EC", "G3-EC", "G2-QT", "G3-QT")         # (the order test_rd_probe_nd's list starts with: one build per workload)


@_on(*RAGGED)
def test_streams_decode_and_index(big):
    _streams_and_decode(big)
    assert big.w.bytes > Z.FOUR_GIB and big.ct > 0


def _boxes(w):
    """In the first period; whole rows across the 4 GiB line (the ragged column edge included); the far corner; the ragged
    rows at the far end with the last whole tiles in front of them; across several periods."""
    sh, rest = w.shape, w.rest
    line_row = LINE // w.row
    zero = (0,) * len(rest)
    inner_lo = tuple(min(1, d - 1) for d in rest)
    inner_hi = tuple(d - 1 for d in rest)
    bx = [((3,) + inner_lo, (w.period - 7,) + inner_hi),
          ((line_row - 9,) + zero, (line_row + 10,) + rest),
          (tuple(d - max(1, d // 80) for d in sh), sh),
          ((sh[0] - w.tail - 3,) + zero, sh),
          ((2 * w.period - 5,) + inner_lo, (4 * w.period + 9,) + tuple(max(l + 1, d // 3) for l, d in zip(inner_lo, rest)))]
    assert (line_row - 9) * w.row < LINE < (line_row + 10) * w.row
    for lo, hi in bx:
        assert all(0 <= l < h <= d for l, h, d in zip(lo, hi, sh)), (lo, hi)
    return bx


def _sl(lo, hi):
    return tuple(slice(l, h) for l, h in zip(lo, hi))


@_on(*RAGGED)
def test_decompress_box_nd_and_boxes_nd(big):
    b, w = big, big.w
    boxes = _boxes(w)
    for lo, hi in boxes:
        r = b.ctx.decompress_box_nd(*b.args(), lo, hi, b.idx, mode=b.mode, qtable=b.q)
        assert Z.same(r, b.full[_sl(lo, hi)].contiguous()), (lo, hi)
        del r
    outs = b.ctx.decompress_boxes_nd(*b.args(), boxes, b.idx, mode=b.mode, qtable=b.q)
    for (lo, hi), r in zip(boxes, outs):
        assert Z.same(r, b.full[_sl(lo, hi)].contiguous()), (lo, hi)


@_on(*RAGGED)
def test_tile_summary_nd(big):
    """Records periodic against the model's, which test_gpu_tile_summary_nd's _check holds to ndsummary_cases' reductions.
    The total: extremes are those of the device's records (and the model's); a sum is held against math.fsum of the device's
    records with ndsummary_cases.bound for any order of summation, here of one term per tile."""
    import torch
    b, w = big, big.w
    model = types.SimpleNamespace(shape=w.model_shape)
    model.want, model.mag, model.m, model.wt, model.mt = NS.reduce(w.model_shape, b.fulls_np, b.s)
    for ref_s, ref_b in ((None, None), (b.sd, b.x)):
        what = f"{w.name} ref={ref_b is not None}"
        recs_s, total_s = b.ctx.tile_summary_nd(*b.args(model=True), index=b.idxs, mode=b.mode, qtable=b.q, ref=ref_s)
        _check_records(recs_s.cpu().numpy(), total_s, model, ref_s is not None, "model of " + what)
        recs, total = b.ctx.tile_summary_nd(*b.args(), index=b.idx, mode=b.mode, qtable=b.q, ref=ref_b)
        assert Z.records_ok(w, recs, recs_s), what
        host = recs.cpu().numpy()
        for f, name in enumerate(NS.FIELDS):
            got, got_s = getattr(total, name), getattr(total_s, name)
            if ref_b is None and f >= 4:
                assert got == 0.0, (what, name)
            elif f in (0, 4):
                assert got == float(torch.min(recs[:, f]).item()) == got_s, (what, name)
            elif f in (1, 5, 6):
                assert got == float(torch.max(recs[:, f]).item()) == got_s, (what, name)
            else:
                exact = math.fsum(host[:, f].tolist())
                bound = NS.bound(w.tiles, math.fsum(np.abs(host[:, f]).tolist()))
                print(f"{what}: total {name} = {got!r}, fsum of the records = {exact!r}, bound = {bound:.3g}")
                assert abs(got - exact) <= bound, (what, name, got, exact, bound)
        if ref_b is not None:
            # (test_gpu_tile_summary_nd.py::test_total_agrees_with_psnr_terms)
            pt = b.ctx.psnr_terms(b.x.view(-1), b.full.view(-1))
            assert (pt[0], pt[1], pt[2]) == (total.xmin, total.xmax, total.emax), (pt, what)
            assert abs(total.esq - pt[3]) <= NS.bound(w.n, math.fsum(host[:, 7].tolist())), (total.esq, pt[3])


@_on(*RAGGED)
def test_fixup_build_nd_and_apply_nd(big):
    b, w = big, big.w
    bound = EB * b.info.sf
    fix_s = b.ctx.fixup_build_nd(*b.args(model=True), b.sd, bound, index=b.idxs, mode=b.mode, qtable=b.q)
    listed, ws, wo, wv = NF.fix_list(b.s, b.fulls_np, bound)
    assert fix_s[3] == wo.size > 0 and np.array_equal(_np_u(fix_s[0], np.uint32), ws)
    assert np.array_equal(_np_u(fix_s[1], np.uint16), wo) and np.array_equal(_np_u(fix_s[2], np.uint64), wv.view(np.uint64))
    count_only = b.ctx.fixup_build_nd(*b.args(), b.x, bound, index=b.idx, mode=b.mode, qtable=b.q, capacity=0)
    assert Z.fix_ok(w, count_only, fix_s)
    fix = b.ctx.fixup_build_nd(*b.args(), b.x, bound, index=b.idx, mode=b.mode, qtable=b.q, capacity=count_only[3])
    assert Z.fix_ok(w, fix, fix_s) and Z.same(fix[0], count_only[0])
    # apply to the whole decode: afterwards !(|x - r| <= bound) holds nowhere (independent of the model) ...
    applied_s = b.ctx.fixup_apply_nd(fix_s, w.model_shape, b.tdt, b.fulls.clone())
    assert np.array_equal(applied_s.cpu().numpy().view(np.uint64), NF.applied(b.s, b.fulls_np, bound).view(np.uint64))
    applied = b.ctx.fixup_apply_nd(fix, w.shape, b.tdt, b.full.clone())
    assert not bool((~((b.x - applied).abs() <= bound)).any().item())
    assert Z.decode_ok(w, applied, applied_s)                                     # ... and nothing else was touched
    # ... and to the far corner and the rows across the 4 GiB line
    for lo, hi in _boxes(w)[1:3]:
        box = b.ctx.decompress_box_nd(*b.args(), lo, hi, b.idx, mode=b.mode, qtable=b.q)
        b.ctx.fixup_apply_nd(fix, w.shape, b.tdt, box, lo=lo, hi=hi)
        assert Z.same(box, applied[_sl(lo, hi)].contiguous()), (lo, hi)


@_on("G2-EC", "G3-EC")
def test_rd_probe_nd(big):
    """16 bounds: every count is reps * cnt_P + cnt_tail exactly, cnt_P and cnt_tail from probing P alone and the model; the
    predicted SSE (over the array's own elements) against the same combination within rd_nd_cases' SSE_RTOL_F64."""
    import torch
    b, w = big, big.w
    pp, rng_p = b.ctx.rd_probe_nd(torch.from_numpy(b.p).to(b.ctx.device), EBS)
    ps, rng_s = b.ctx.rd_probe_nd(b.sd, EBS)
    for eb in PROBE_ORACLE:
        c = O.compress_nd(b.s, eb, H.EC, O.FAST)
        a, s = pp[EBS.index(eb)], ps[EBS.index(eb)]
        assert (a["cnt"], s["cnt"] - a["cnt"]) == Z.period_counts(c.bin_index, w) and s["cnt"] == c.cnt, eb
    pb, rng_b = b.ctx.rd_probe_nd(b.x, EBS)
    assert rng_b == rng_s == rng_p == (float(b.s.min()), float(b.s.max()))
    assert Z.probe_ok(w, [v["cnt"] for v in pb], [v["cnt"] for v in pp], [v["cnt"] for v in ps])
    assert pb[EBS.index(EB)]["cnt"] == b.info.cnt
    want = Z.probe_counts(w, [v["sse"] for v in pp], [v["sse"] for v in ps])
    for eb, v, sse in zip(EBS, pb, want):
        assert v["error_bound"] == eb
        assert abs(v["sse"] - sse) <= SSE_RTOL_F64 * sse, (eb, v["sse"], sse)


@_on("G2-holes", "G3-holes")
def test_mask_build_nd_and_compress_masked_nd(big):
    """Words, filled copy (inside each tile) and count predicted from the model, which is held to ndmask_cases' numpy fill."""
    import torch
    b, w, ctx = big, big.w, big.ctx
    miss_s = M.is_missing(b.s, FLAGS, VALUE, LIMIT)
    want_f = NM.fill(b.s, miss_s)
    mask_s, count_s, filled_s = ctx.mask_build_nd(b.sd, FLAGS, VALUE, LIMIT)
    assert count_s == int(miss_s.sum()) > 0 and np.array_equal(_np_u(mask_s, np.uint64), NM.mask_words(miss_s))
    assert np.array_equal(_np_u(filled_s, np.uint64), want_f.reshape(-1).view(np.uint64))
    mask, count, filled = ctx.mask_build_nd(b.x, FLAGS, VALUE, LIMIT)
    assert Z.mask_ok(w, mask, count, mask_s, count_s) and Z.decode_ok(w, filled, filled_s)
    assert count == int((torch.isnan(b.x) | (b.x.abs() >= LIMIT)).sum().item())   # (Inf included; independent of the model)
    x2 = b.x.clone()
    mask2, count2, f2 = ctx.mask_build_nd(x2, FLAGS, VALUE, LIMIT, filled=x2)     # in place
    assert count2 == count and Z.same(mask2, mask) and Z.same(x2, filled)
    del x2, f2
    mask3, count3, f3 = ctx.mask_build_nd(b.x, FLAGS, VALUE, LIMIT, filled=False)  # mask only
    assert f3 is None and count3 == count and Z.same(mask3, mask)
    # compress_masked_nd: the mask, the filled copy, and the streams of the filled array
    c = O.compress_nd(want_f, EB, H.EC, O.FAST)
    fs = torch.empty_like(b.sd)
    outs, infos, ms, ks = ctx.compress_masked_nd(b.sd, EB, FLAGS, VALUE, LIMIT, filled=fs)
    assert (infos.sf, infos.cnt, ks) == (c.sf, c.cnt, count_s) and Z.same(ms, mask_s) and Z.same(fs, filled_s)
    assert np.array_equal(_np_u(outs["bin_index"], np.uint8), c.bin_index)
    assert np.array_equal(_np_u(outs["dc"], np.uint32), c.dc.view(np.uint32))
    assert np.array_equal(_np_u(outs["ac_exact"][:c.cnt], np.uint32), c.ac_exact.view(np.uint32))
    fb = torch.empty_like(b.x)
    out, info, mb, kb = ctx.compress_masked_nd(b.x, EB, FLAGS, VALUE, LIMIT, filled=fb)
    assert (info.sf, info.max_abs, info.min_abs) == (infos.sf, infos.max_abs, infos.min_abs) and kb == count
    assert Z.same(mb, mask) and Z.same(fb, filled)
    assert Z.streams_ok(w, out, info.cnt, outs, infos.cnt)
