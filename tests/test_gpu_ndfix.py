"""Point-wise error bound for arrays compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h: dctzhip_fixup_build_nd /
dctzhip_fixup_apply_nd): the list over the stream positions, built against the array in place, and its application to the
output of a whole or box decode.

Reference: the device's own decompress_nd of the same streams (code from before this layer) through the numpy restatement of
the definition in tests/ndfix_cases.py; everything is compared exactly.  Shapes, fields, bounds and what each shape is for:
tests/ndfix_cases.py; that none of the cases is vacuous is asserted on the CPU (tests/test_ndfix_cases_cpu.py) and again
here from the device's decode."""
import ctypes as C

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import ndfix_cases as N

pytestmark = pytest.mark.gpu

EB = N.EB
GUARD = 64                            # sentinel elements on either side of a buffer (keeps the middle 16-byte aligned)
CASES = [(s, dt, mode, kind) for s in N.SHAPES for dt in (np.float64, np.float32) for mode in (H.EC, H.QT) for kind in N.KINDS]


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
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def _banded(ctx, src, tdt, fill):
    """src (numpy) between two bands of `fill` on the device: (buffer, the contiguous view of the middle shaped like src)."""
    import torch
    buf = torch.full((src.size + 2 * GUARD,), fill, dtype=tdt, device=ctx.device)
    mid = buf[GUARD:GUARD + src.size].view(src.shape)
    mid.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return buf, mid


def _bands_are(buf, fill):
    b = buf.cpu().numpy()
    want = _bits(np.array([fill], dtype=b.dtype))[0]
    return bool((_bits(b[:GUARD]) == want).all() and (_bits(b[-GUARD:]) == want).all())


SENT = -7.25e11


class Streams:
    """One array on the device with its streams, index, table and full decode.  The original sits between bands of NaN: a
    read past a ragged edge, or in front of the array, would list entries the definition does not have."""

    def __init__(self, ctx, x, mode):
        self.x, self.shape, self.mode, self.dtype = x, tuple(x.shape), mode, x.dtype.type
        self.tdt = _tdt(x.dtype)
        self.buf, self.xd = _banded(ctx, x, self.tdt, float("nan"))
        self.out, self.info = ctx.compress_nd(self.xd, EB, mode)
        self.q = np.array(self.info.qtable[:]) if mode == H.QT else None
        self.sf, self.cnt = self.info.sf, self.info.cnt
        self.full_d = ctx.decompress_nd(self.out, self.cnt, self.shape, self.tdt, EB, self.sf, mode, qtable=self.q)
        self.full = self.full_d.cpu().numpy()
        self.idx, tot = ctx.ac_index(self.out, 64 * N.nblk(self.shape))
        assert tot == self.cnt

    def build(self, ctx, bound, **kw):
        return ctx.fixup_build_nd(self.out, self.cnt, self.shape, self.tdt, EB, self.sf, self.xd, bound, index=self.idx, mode=self.mode,
                                  qtable=self.q, **kw)

    def raw_build(self, ctx, bound, start, off, val, cap, count, **kw):
        q = np.ascontiguousarray(self.q, dtype=self.dtype) if self.q is not None else None
        ptr = lambda v: v if v is None or isinstance(v, int) else v.data_ptr()
        a = dict(bin=self.out["bin_index"], dc=self.out["dc"], ac=self.out["ac_exact"], idx=self.idx, ref=self.xd, dims=self.shape, cnt=self.cnt,
                 q=q, countp=C.byref(count))
        a.update(kw)
        dims = None if a["dims"] is None else (C.c_size_t * len(a["dims"]))(*a["dims"])
        return ctx.lib.dctzhip_fixup_build_nd(
            ctx.h, ptr(a["bin"]), ptr(a["dc"]), ptr(a["ac"]), int(a["cnt"]), ptr(a["idx"]),
            a["q"].ctypes.data_as(C.c_void_p) if a["q"] is not None else None, 0 if dims is None else len(a["dims"]), dims, H._dt(self.tdt), EB,
            float(self.sf), self.mode, ptr(a["ref"]), float(bound), ptr(start), ptr(off), ptr(val), int(cap), a["countp"])

    def expect(self, bound):
        return N.fix_list(self.x, self.full, bound)

    def applied(self, bound):
        return N.applied(self.x, self.full, bound)


def _fix_np(fix):
    start, off, val, count = fix
    s = start.cpu().numpy().view(np.uint32)
    if off is None:
        return s, None, None, count
    return s, off.cpu().numpy().view(np.uint16), val.cpu().numpy(), count


def _same_list(fix, want, what):
    s, o, v, k = _fix_np(fix)
    _, ws, wo, wv = want
    assert k == int(ws[-1]) == wo.size, (what, k, int(ws[-1]))
    assert np.array_equal(s, ws), what
    assert o.size == k and np.array_equal(o, wo), what
    assert v.size == k and np.array_equal(_bits(v), _bits(wv)), what


_DATA = {}


def _data(ctx, shape, dtype, mode, kind):
    key = (shape, np.dtype(dtype).name, mode, kind)
    if key not in _DATA:
        _DATA[key] = Streams(ctx, N.field(shape, kind, dtype), mode)
    return _DATA[key]


def _mark_name(dtype, mode, shape):
    return f"k_ndfix_mark<{'double' if dtype == np.float64 else 'float'}, {mode}, {len(shape) - 1}>"


def _apply_name(dtype, shape):
    return f"k_ndfix_apply<{'double' if dtype == np.float64 else 'float'}, {len(shape) - 1}>"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_build_gives_the_list_of_the_definition(ctx, case):
    """fix_start, fix_off, fix_val and count equal the restatement exactly; the count-only form gives the same table; a second
    call gives the same bytes; the mark kernel is named."""
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    assert s.sf == 100.0
    counts = []
    for m in N.MULTS:
        b = m * EB * s.sf
        what = f"{_id(case)} m={m}"
        want = s.expect(b)
        fix = s.build(ctx, b)
        assert ctx.last_kernel(1) == _mark_name(dtype, mode, shape)
        _same_list(fix, want, what)
        start0, off0, val0, k0 = s.build(ctx, b, capacity=0)
        assert off0 is None and val0 is None and k0 == fix[3], what
        assert np.array_equal(start0.cpu().numpy().view(np.uint32), want[1]), what
        if fix[3]:
            again = s.build(ctx, b, capacity=fix[3])
            for a_, b_ in zip(_fix_np(again)[:3], _fix_np(fix)[:3]):
                assert np.array_equal(_bits(a_), _bits(b_)), what
        counts.append(fix[3])
    print(f"{_id(case)}: listed for m = {N.MULTS}: {counts}")
    assert counts[0] > 0 and counts == sorted(counts, reverse=True) and counts[-1] == 0
    if kind == "noisy" and N.has_full_tile(shape):
        per = np.diff(s.expect(N.MULTS[0] * EB * s.sf)[1].astype(np.int64))
        rp = np.zeros(N.tiles(shape) * N.TILE, bool)
        rp[:64 * N.nblk(shape)] = N.real(shape)
        assert (2 * per > rp.reshape(-1, N.TILE).sum(axis=1)).any(), per


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "noisy"], ids=_id)
def test_a_list_that_does_not_fit_is_counted_and_not_written(ctx, case):
    import torch
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    b = 0.25 * EB * s.sf
    want = s.expect(b)
    k = int(want[1][-1])
    assert k >= 2
    start = torch.zeros(want[1].size, dtype=torch.int32, device=ctx.device)
    obuf = torch.full((k + 2 * GUARD,), 0x5a5a, dtype=torch.int16, device=ctx.device)
    vbuf = torch.full((k + 2 * GUARD,), SENT, dtype=s.tdt, device=ctx.device)
    off, val = obuf[GUARD:GUARD + k], vbuf[GUARD:GUARD + k]
    o0, v0 = obuf.cpu().numpy().copy(), vbuf.cpu().numpy().copy()
    count = C.c_uint32(0)
    assert s.raw_build(ctx, b, start, off, val, k - 1, count) == H.E_SPACE
    assert count.value == k
    assert np.array_equal(start.cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(obuf.cpu().numpy(), o0) and np.array_equal(_bits(vbuf.cpu().numpy()), _bits(v0))
    # the same buffers with room: the list, and the bands around it untouched
    assert s.raw_build(ctx, b, start, off, val, k, count) == H.OK and count.value == k
    _same_list((start, off, val, k), want, _id(case))
    assert np.array_equal(obuf.cpu().numpy()[:GUARD], o0[:GUARD]) and np.array_equal(obuf.cpu().numpy()[-GUARD:], o0[-GUARD:])
    assert _bands_are(vbuf, SENT)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_apply_to_the_whole_array(ctx, case):
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    for m in N.MULTS:
        b = m * EB * s.sf
        fix = s.build(ctx, b)
        buf, mid = _banded(ctx, s.full, s.tdt, SENT)
        ctx.fixup_apply_nd(fix, shape, s.tdt, mid)
        assert ctx.last_kernel(1) == _apply_name(dtype, shape)
        got = mid.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(s.applied(b))), (_id(case), m)
        assert N.guarantee_holds(s.x, got, b), (_id(case), m)
        assert _bands_are(buf, SENT)


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "noisy"], ids=_id)
def test_apply_to_boxes(ctx, case):
    """The output of decompress_box_nd becomes the slice of the whole-array result; the bands around it stay."""
    shape, dtype, mode, kind = case
    s = _data(ctx, shape, dtype, mode, kind)
    b = 0.5 * EB * s.sf
    fix = s.build(ctx, b)
    assert fix[3] > 0
    whole = s.applied(b)
    touched = 0
    for lo, hi in N.boxes(shape):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        ext = [h - l for l, h in zip(lo, hi)]
        buf, mid = _banded(ctx, np.zeros(ext, dtype), s.tdt, SENT)
        ctx.decompress_box_nd(s.out, s.cnt, shape, s.tdt, EB, s.sf, lo, hi, s.idx, mode, qtable=s.q, dst=mid)
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(s.full[sl])), (lo, hi)
        ctx.fixup_apply_nd(fix, shape, s.tdt, mid, lo=lo, hi=hi)
        got = mid.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(whole[sl])), (_id(case), lo, hi)
        assert N.guarantee_holds(s.x[sl], got, b), (lo, hi)
        assert _bands_are(buf, SENT), (lo, hi)
        touched += int((_bits(whole[sl]) != _bits(s.full[sl])).sum())
    assert touched > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_more_tiles_than_resident_workgroups(ctx, dtype):
    """(256, 256, 160): 2560 stream tiles, the grid-stride loops of all three kernels."""
    s = Streams(ctx, N.field(N.BIG, "noisy", dtype), H.EC)
    assert N.tiles(N.BIG) == 2560
    b = 1.0 * EB * s.sf
    want = s.expect(b)
    assert 0 < int(want[1][-1]) < s.x.size
    fix = s.build(ctx, b)
    _same_list(fix, want, "big")
    buf, mid = _banded(ctx, s.full, s.tdt, SENT)
    ctx.fixup_apply_nd(fix, N.BIG, s.tdt, mid)
    got = mid.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(s.applied(b))) and N.guarantee_holds(s.x, got, b) and _bands_are(buf, SENT)
    lo, hi = (10, 100, 30), (20, 110, 150)
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    box = ctx.decompress_box_nd(s.out, s.cnt, N.BIG, s.tdt, EB, s.sf, lo, hi, s.idx, H.EC)
    ctx.fixup_apply_nd(fix, N.BIG, s.tdt, box, lo=lo, hi=hi)
    assert np.array_equal(_bits(box.cpu().numpy()), _bits(s.applied(b)[sl]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_nan_lists_its_tile_and_stays_a_nan(ctx, dtype):
    """A NaN in an interior 8 x 8 tile lists its 64 positions; one in the bottom-right tile of (45, 77) -- 5 x 5 real positions --
    lists those 25 and no padded one.  Both stay NaN after apply, their neighbours get the original back.  (The field is scaled
    to |x| < 100 as tests/nonfinite.py asks of an array that receives a NaN.)"""
    shape = (45, 77)
    x = N.field(shape, "smooth", dtype) * dtype(0.09)
    x[20, 35] = np.nan                                   # block (2, 4): interior
    x[44, 76] = np.nan                                   # block (5, 9): rows 40 .. 44, columns 72 .. 76
    s = Streams(ctx, x, H.EC)
    bad = np.zeros(shape, bool)
    bad[16:24, 32:40] = True
    bad[40:45, 72:77] = True
    assert np.array_equal(np.isnan(s.full), bad)
    b = 4.0 * EB * s.sf
    lm, start, off, val = want = s.expect(b)
    assert lm[bad].all()
    fix = s.build(ctx, b)
    _same_list(fix, want, "nan")
    blk = (int(start[0]) + off.astype(np.int64)) >> 6     # one stream tile: the offset is the position
    assert N.tiles(shape) == 1 and int((blk == 2 * 10 + 4).sum()) == 64 and int((blk == 5 * 10 + 9).sum()) == 25
    buf, mid = _banded(ctx, s.full, s.tdt, SENT)
    ctx.fixup_apply_nd(fix, shape, s.tdt, mid)
    got = mid.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(s.applied(b))) and _bands_are(buf, SENT)
    assert np.isnan(got[20, 35]) and np.isnan(got[44, 76]) and int(np.isnan(got).sum()) == 2
    assert np.array_equal(_bits(got[bad]), _bits(x[bad]))
    assert N.guarantee_holds(x, got, b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_nan_in_a_3d_edge_tile(ctx, dtype):
    shape = (13, 22, 35)
    x = N.field(shape, "smooth", dtype) * dtype(0.09)
    x[12, 21, 34] = np.nan                               # the last block: 1 x 2 x 3 real positions
    s = Streams(ctx, x, H.EC)
    assert int(np.isnan(s.full).sum()) == 6
    b = 4.0 * EB * s.sf
    want = s.expect(b)
    assert want[0][12:, 20:, 32:].all()
    fix = s.build(ctx, b)
    _same_list(fix, want, "nan 3-D")
    last = N.nblk(shape) - 1
    q = (N.tiles(shape) - 1) * N.TILE + want[2][int(want[1][-2]):].astype(np.int64)
    assert int((q >> 6 == last).sum()) == 6
    got = ctx.fixup_apply_nd(fix, shape, s.tdt, s.full_d.clone()).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(s.applied(b))) and int(np.isnan(got).sum()) == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_build_refusals_leave_the_context_usable(ctx, dtype, mode):
    import torch
    shape = (16, 520)
    s = _data(ctx, shape, dtype, mode, "noisy")
    b = 0.5 * EB * s.sf
    want = s.expect(b)
    k = int(want[1][-1])
    es = 8 if dtype == np.float64 else 4
    start = torch.zeros(want[1].size, dtype=torch.int32, device=ctx.device)
    off = torch.zeros(k, dtype=torch.int16, device=ctx.device)
    val = torch.zeros(k, dtype=s.tdt, device=ctx.device)
    count = C.c_uint32(0)

    def after():
        assert s.raw_build(ctx, b, start, off, val, k, count) == H.OK and count.value == k
        _same_list((start, off, val, k), want, "after a refusal")

    after()
    big = 1 << 40
    refused = [
        dict(ref=0), dict(ref=s.xd.data_ptr() + es), dict(countp=None),
        dict(bin=0), dict(bin=s.out["bin_index"].data_ptr() + 4), dict(dc=0), dict(dc=s.out["dc"].data_ptr() + 2), dict(idx=0),
        dict(idx=s.idx.data_ptr() + 2), dict(ac=0), dict(ac=s.out["ac_exact"].data_ptr() + 2),
        dict(dims=None), dict(dims=(16,)), dict(dims=(16, 520, 1, 1)), dict(dims=(16, 0)), dict(dims=(big, big)),
    ]
    if mode == H.QT:
        refused.append(dict(q=None))
    for kw in refused:
        assert s.raw_build(ctx, b, start, off, val, k, count, **kw) == H.E_ARG, kw
        after()
    for bad in (-1.0, float("nan"), float("inf")):
        assert s.raw_build(ctx, bad, start, off, val, k, count) == H.E_ARG, bad
    after()
    # the outputs: fix_start missing or misaligned, one of the pair missing, misaligned, overlapping an input or each other
    assert s.raw_build(ctx, b, 0, off, val, k, count) == H.E_ARG
    assert s.raw_build(ctx, b, start.data_ptr() + 2, off, val, k, count) == H.E_ARG
    assert s.raw_build(ctx, b, start, None, val, k, count) == H.E_ARG
    assert s.raw_build(ctx, b, start, off, None, k, count) == H.E_ARG
    assert s.raw_build(ctx, b, start, off.data_ptr() + 1, val, k - 1, count) == H.E_ARG
    assert s.raw_build(ctx, b, start, off, val.data_ptr() + 2, k - 1, count) == H.E_ARG
    assert s.raw_build(ctx, b, s.idx, off, val, k, count) == H.E_ARG                         # fix_start over the index
    assert s.raw_build(ctx, b, start, off, s.xd, min(k, s.x.size), count) == H.E_ARG          # fix_val over the original
    assert s.raw_build(ctx, b, start, off, start, 1, count) == H.E_ARG                         # fix_val over fix_start
    after()
    # a damaged index: DCTZHIP_E_ARG from the kernel's own check, and a clean next call
    for t in (0, 1, N.tiles(shape)):
        ix = s.idx.clone()
        ix[t] += 1
        assert s.raw_build(ctx, b, start, off, val, k, count, idx=ix) == H.E_ARG, t
        after()
    assert s.raw_build(ctx, b, start, off, val, k, count, cnt=s.cnt - 1) == H.E_ARG
    after()


def _raw_apply(ctx, s, start, off, val, count, mid, lo=None, hi=None, dims=None):
    dims = s.shape if dims is None else dims
    lo = [0] * len(dims) if lo is None else lo
    hi = list(dims) if hi is None else hi
    arr = lambda v: (C.c_size_t * len(v))(*v)
    ptr = lambda v: v if v is None or isinstance(v, int) else v.data_ptr()
    return ctx.lib.dctzhip_fixup_apply_nd(ctx.h, ptr(start), ptr(off), ptr(val), int(count), len(dims), arr(dims), H._dt(s.tdt), arr(lo), arr(hi),
                                          ptr(mid))


TAMPER = [((16, 520), np.float64, H.EC), ((16, 520), np.float32, H.QT), ((13, 22, 35), np.float64, H.QT), ((13, 22, 35), np.float32, H.EC)]


@pytest.mark.parametrize("case", TAMPER, ids=lambda c: _id((c[0], c[1], c[2], "noisy")))
def test_apply_refuses_a_tampered_list(ctx, case):
    """Each way a list can contradict itself or the array, on shapes with nblk % 64 != 0 and ragged edges: DCTZHIP_E_ARG, the
    refused tile stores nothing, nothing outside the box is written, and the next good call is clean."""
    import torch
    shape, dtype, mode = case
    s = _data(ctx, shape, dtype, mode, "noisy")
    nblk, m = N.nblk(shape), N.tiles(shape)
    assert nblk % 64 != 0 and m >= 3 and (shape != (13, 22, 35) or not N.real(shape).all())
    b = 0.25 * EB * s.sf
    start, off, val, k = s.build(ctx, b)
    ws = start.cpu().numpy().view(np.uint32).astype(np.int64)
    wo = off.cpu().numpy().view(np.uint16).astype(np.int64)
    good = s.applied(b)
    last = m - 1
    assert all(ws[t + 1] - ws[t] >= 3 for t in range(m))

    def run(st=None, of=None, cnt=None, lo=None, hi=None):
        sl = tuple(slice(0, d) for d in shape) if lo is None else tuple(slice(l, h) for l, h in zip(lo, hi))
        buf, mid = _banded(ctx, s.full[sl], s.tdt, SENT)
        stt = start if st is None else torch.from_numpy(np.asarray(st, dtype=np.uint32).view(np.int32)).to(ctx.device)
        oft = off if of is None else torch.from_numpy(np.asarray(of, dtype=np.uint16).view(np.int16)).to(ctx.device)
        rc = _raw_apply(ctx, s, stt, oft, val, k if cnt is None else cnt, mid, lo, hi)
        assert _bands_are(buf, SENT)
        return rc, mid.cpu().numpy(), sl

    def untouched_tile(got, t):
        """No position of stream tile t was stored: the output there still has the decode's bits."""
        q = np.arange(t * N.TILE, min((t + 1) * N.TILE, 64 * nblk))
        c = N.coords(shape, q)
        ok = np.ones(q.size, bool)
        for a, d in enumerate(shape):
            ok &= c[a] < d
        at = tuple(v[ok] for v in c)
        return np.array_equal(_bits(got[at]), _bits(s.full[at]))

    def clean():
        rc, got, _ = run()
        assert rc == H.OK and np.array_equal(_bits(got), _bits(good))

    clean()
    # the table: not monotone, beyond count, more entries than the tile holds
    st = ws.copy(); st[1] = st[2] + 1
    rc, got, _ = run(st=st); assert rc == H.E_ARG and untouched_tile(got, 0) and untouched_tile(got, 1)
    clean()
    st = ws.copy(); st[1:] += 5
    rc, got, _ = run(st=st); assert rc == H.E_ARG
    rc, got, _ = run(cnt=k - 1); assert rc == H.E_ARG                               # fix_start[m] != count
    rc, got, _ = run(cnt=k + 1); assert rc == H.E_ARG
    clean()
    # offsets: not strictly ascending (equal, swapped), in tile 1
    for i, j in ((ws[1], ws[1] + 1), (ws[1] + 1, ws[1] + 2)):
        of = wo.copy(); of[j] = of[i]
        rc, got, _ = run(of=of); assert rc == H.E_ARG and untouched_tile(got, 1)
    of = wo.copy(); of[ws[1]], of[ws[1] + 1] = wo[ws[1] + 1], wo[ws[1]]
    rc, got, _ = run(of=of); assert rc == H.E_ARG and untouched_tile(got, 1)
    clean()
    # an offset in a block >= nblk: the last entry of the last tile moved behind the array's last block
    assert 64 * (nblk % 64) < N.TILE
    of = wo.copy(); of[k - 1] = 64 * (nblk % 64) + 1
    rc, got, _ = run(of=of); assert rc == H.E_ARG and untouched_tile(got, last)
    of = wo.copy(); of[k - 1] = N.TILE - 1
    rc, got, _ = run(of=of); assert rc == H.E_ARG and untouched_tile(got, last)
    clean()
    # an offset at a padded position: an entry moved onto the nearest padded position behind its neighbour in front
    pad = ~N.real(shape)
    moved = 0
    for t in range(m):
        lo_i, hi_i = int(ws[t]), int(ws[t + 1])
        for i in range(lo_i, hi_i):
            prev = wo[i - 1] if i > lo_i else -1
            nxt = wo[i + 1] if i + 1 < hi_i else min(N.TILE, 64 * nblk - t * N.TILE)
            cand = [o for o in range(prev + 1, nxt) if pad[t * N.TILE + o]]
            if cand:
                of = wo.copy(); of[i] = cand[0]
                rc, got, _ = run(of=of)
                assert rc == H.E_ARG and untouched_tile(got, t), (t, i, cand[0])
                moved += 1
                break
    assert moved >= 1 or pad.sum() == 0
    clean()
    # a box: a tampered tile outside the candidate tiles is not visited; inside, it is refused and nothing outside the box written
    lo, hi = [0] * len(shape), [min(d, 4) for d in shape]
    of = wo.copy(); of[k - 1] = N.TILE - 1                                          # damage in the last tile
    rc, got, sl = run(of=of, lo=lo, hi=hi)
    first_only = N.position(shape, [h - 1 for h in hi]) // N.TILE < last
    assert first_only and rc == H.OK and np.array_equal(_bits(got), _bits(good[sl]))
    lo = [max(0, d - 3) for d in shape]
    rc, got, sl = run(of=of, lo=lo, hi=list(shape)); assert rc == H.E_ARG
    clean()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_apply_refuses_an_entry_at_a_padded_position(ctx, dtype):
    """(45, 77), one stream tile of 60 blocks, ragged on both axes: every listed entry that has a padded position between itself
    and its neighbour in front is moved there in turn (up to 40 of them); each time the call is refused and stores nothing."""
    import torch
    shape = (45, 77)
    s = _data(ctx, shape, dtype, H.QT, "noisy")
    start, off, val, k = s.build(ctx, 0.25 * EB * s.sf)
    wo = off.cpu().numpy().view(np.uint16).astype(np.int64)
    pad = ~N.real(shape)
    assert N.tiles(shape) == 1 and pad.any()
    tried = 0
    for i in range(k):
        cand = [o for o in range(int(wo[i - 1]) + 1 if i else 0, int(wo[i])) if pad[o]]
        if not cand or tried >= 40:
            continue
        of = wo.copy(); of[i] = cand[-1]
        buf, mid = _banded(ctx, s.full, s.tdt, SENT)
        oft = torch.from_numpy(of.astype(np.uint16).view(np.int16)).to(ctx.device)
        assert _raw_apply(ctx, s, start, oft, val, k, mid) == H.E_ARG, (i, cand[-1])
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(s.full)) and _bands_are(buf, SENT)
        tried += 1
    assert tried >= 5
    buf, mid = _banded(ctx, s.full, s.tdt, SENT)
    assert _raw_apply(ctx, s, start, off, val, k, mid) == H.OK
    assert np.array_equal(_bits(mid.cpu().numpy()), _bits(s.applied(0.25 * EB * s.sf)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_apply_host_refusals(ctx, dtype):
    import torch
    shape = (45, 77)
    s = _data(ctx, shape, dtype, H.EC, "noisy")
    start, off, val, k = s.build(ctx, 0.5 * EB * s.sf)
    mid = s.full_d.clone()
    n = s.x.size
    assert _raw_apply(ctx, s, start, off, val, k, mid) == H.OK
    for kw in (dict(dims=(45,)), dict(dims=(45, 77, 1, 1)), dict(dims=(45, 0)), dict(lo=[0, 0], hi=[46, 77]), dict(lo=[5, 0], hi=[5, 77]),
               dict(lo=[0, 78], hi=[45, 77])):
        assert _raw_apply(ctx, s, start, off, val, k, mid, **kw) == H.E_ARG, kw
    assert _raw_apply(ctx, s, None, off, val, k, mid) == H.E_ARG
    assert _raw_apply(ctx, s, start, None, val, k, mid) == H.E_ARG
    assert _raw_apply(ctx, s, start, off, None, k, mid) == H.E_ARG
    assert _raw_apply(ctx, s, start, off, val, k, None) == H.E_ARG
    assert _raw_apply(ctx, s, start, off, val, n + 1, mid) == H.E_ARG                  # more entries than real positions
    assert _raw_apply(ctx, s, start, off, val, k, val) == H.E_ARG                      # d_out over the list
    assert _raw_apply(ctx, s, start, off, val, k, mid) == H.OK
    assert np.array_equal(_bits(mid.cpu().numpy()), _bits(s.applied(0.5 * EB * s.sf)))


@pytest.mark.parametrize("shape", [(45, 77), (64, 512)], ids=["45x77", "64x512"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_composition_with_the_mask_layer(ctx, shape, dtype):
    """Existing mask calls serve tiles as they are, because the mask's bits follow the C-order array: mask_build on the flattened
    holey array, compress_nd of the filled copy, the list against the filled copy; then box decode, fixup_apply_nd,
    mask_apply(dims=shape).  Valid elements have the original's bits or lie within the bound, missing ones the fill's bits."""
    import torch
    tdt = _tdt(dtype)
    x = N.field(shape, "noisy", dtype)
    rng = np.random.default_rng(3)
    holes = rng.random(shape) < 0.05
    holes[-1, -1] = True
    holes[0, :9] = True
    x[holes] = np.nan
    n = x.size
    xd = torch.from_numpy(x).to(ctx.device)
    mask, count, filled = ctx.mask_build(xd.view(-1), H.MISS_NAN)
    assert count == int(holes.sum())
    filled = filled.view(shape)
    fx = filled.cpu().numpy()
    assert not np.isnan(fx).any()
    out, info = ctx.compress_nd(filled, EB, H.EC)
    idx, _ = ctx.ac_index(out, 64 * N.nblk(shape))
    b = 0.5 * EB * info.sf
    fix = ctx.fixup_build_nd(out, info.cnt, shape, tdt, EB, info.sf, filled, b, index=idx)
    assert fix[3] > 0
    fill = dtype(-9999.0)
    for lo, hi in N.boxes(shape):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        box = ctx.decompress_box_nd(out, info.cnt, shape, tdt, EB, info.sf, lo, hi, idx, H.EC)
        ctx.fixup_apply_nd(fix, shape, tdt, box, lo=lo, hi=hi)
        ctx.mask_apply(mask, n, float(fill), box, dims=shape, lo=lo, hi=hi)
        got = box.cpu().numpy()
        h = holes[sl]
        assert np.array_equal(_bits(got[h]), _bits(np.full(int(h.sum()), fill, dtype)))
        assert N.guarantee_holds(fx[sl][~h], got[~h], b), (lo, hi)
