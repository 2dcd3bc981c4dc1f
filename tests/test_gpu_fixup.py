"""Point-wise error bound (include/dctz_hip.h: dctzhip_fixup_build / dctzhip_fixup_apply): the list of the elements whose
reconstruction misses the original by more than a bound, built beside the streams, and its application to the output of a
whole, range or box decode.

Reference: the library's own ctx.decompress of the same streams, in numpy: mask = ~(abs(x - full) <= dtype(b)), its per-tile
prefix, the offsets in the tile and x[mask] as bits.  Everything is compared exactly.

Fields and sizes are those of tests/test_gpu_tile_summary.py; bounds are m EB sf for m in 0.25, 0.5, 1, 2.  The CPU oracle
gives these counts for fp64 EC (fp32 and QT within four), so dense, sparse, few-entry and empty lists and the short block
are all reached:

    n       kind     m = 0.25                   0.5                       1                      2
    12645   noisy    7657 (23 short block)      3770 (12 short block)     428 (2 short block)    0
    12645   smooth   562 (3 short block)        9                         0                      0
    4096    noisy    2406                       1190                      155                    0
    4097    noisy    2499                       1201                      134                    0
    37      noisy    23                         9                         2                      0
    37      smooth   6                          0                         0                      0
"""
import ctypes as C

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import dropin_cases as D
from tests import nonfinite as NF

pytestmark = pytest.mark.gpu

EB = 1e-3
TILE = 4096
MULTS = (0.25, 0.5, 1.0, 2.0)
FLAT_N = [37, 4096, 4097, 3 * 4096 + 5 * 64 + 37]
BIG_N = 2051 * 4096 + 100            # above any resident grid of single-wave workgroups on 256 CUs: the grid-stride loops
CASES = [(n, dt, mode, kind) for n in FLAT_N for dt in (np.float64, np.float32) for mode in (H.EC, H.QT) for kind in ("smooth", "noisy")]
GUARD = 64                            # sentinel elements on either side of an output


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
    """tests/test_gpu_tile_summary.py's field: sf = 100; smooth stores nothing exactly, noisy about three coefficients in ten."""
    i = np.arange(n, dtype=np.float64)
    x = 100.0 + 60.0 * np.sin(i / 4000.0) + 6.0 * np.cos(i / 1000.0)
    if kind == "noisy":
        x = x + 25.0 * np.clip(np.random.default_rng(seed).standard_normal(n), -4.0, 4.0)
    return x.astype(dtype)


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32 if a.dtype.itemsize == 4 else np.uint16)


class Streams:
    """One array on the device with its streams, index, table and full decode."""

    def __init__(self, ctx, x, mode):
        import torch
        self.x, self.n, self.mode, self.dtype = x, x.size, mode, x.dtype.type
        self.tdt = _tdt(x.dtype)
        self.xd = torch.from_numpy(x).to(ctx.device)
        self.out, self.info = ctx.compress(self.xd, EB, mode)
        self.q = np.array(self.info.qtable[:]) if mode == H.QT else None
        self.sf, self.cnt = self.info.sf, self.info.cnt
        self.full = ctx.decompress(self.out, self.cnt, self.n, self.tdt, EB, self.sf, mode, qtable=self.q).cpu().numpy()
        self.idx, tot = ctx.ac_index(self.out, self.n)
        assert tot == self.cnt

    def build(self, ctx, bound, **kw):
        return ctx.fixup_build(self.out, self.cnt, self.n, self.tdt, EB, self.sf, self.xd, bound, index=self.idx, mode=self.mode, qtable=self.q, **kw)

    def raw_build(self, ctx, bound, start, off, val, cap, count, ref=-1, idx=None):
        q = np.ascontiguousarray(self.q, dtype=self.dtype) if self.q is not None else None
        return ctx.lib.dctzhip_fixup_build(
            ctx.h, self.out["bin_index"].data_ptr(), self.out["dc"].data_ptr(), self.out["ac_exact"].data_ptr(), int(self.cnt),
            (self.idx if idx is None else idx).data_ptr(), q.ctypes.data_as(C.c_void_p) if q is not None else None, self.n, H._dt(self.tdt), EB,
            float(self.sf), self.mode, self.xd.data_ptr() if ref == -1 else ref, float(bound), start.data_ptr(),
            off.data_ptr() if off is not None else None, val.data_ptr() if val is not None else None, int(cap), C.byref(count))

    def expect(self, bound):
        """(mask, fix_start, fix_off, fix_val) of the definition, from the full decode."""
        with np.errstate(invalid="ignore"):
            mask = ~(np.abs(self.x - self.full) <= self.dtype(bound))
        tiles = -(-self.n // TILE)
        per = np.array([int(mask[t * TILE:(t + 1) * TILE].sum()) for t in range(tiles)], dtype=np.uint64)
        start = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
        at = np.flatnonzero(mask)
        return mask, start, (at % TILE).astype(np.uint16), self.x[at]

    def applied(self, bound):
        mask = self.expect(bound)[0]
        return np.where(mask, self.x, self.full)


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


def _guarantee(x, out, bound, what):
    """Every element has the bits of x or lies within the bound of it (section 1 of the contract)."""
    same = _bits(out) == _bits(x)
    with np.errstate(invalid="ignore"):
        near = np.abs(x - out) <= x.dtype.type(bound)
    assert bool((same | near).all()), (what, int((~(same | near)).sum()))


_DATA = {}


def _data(ctx, n, dtype, mode, kind):
    key = (n, np.dtype(dtype).name, mode, kind)
    if key not in _DATA:
        _DATA[key] = Streams(ctx, _field(n, kind, dtype, seed=n), mode)
    return _DATA[key]


def _guarded(ctx, s, src):
    """src (numpy) between two bands of sentinels on the device: (buffer, the view of the middle, the sentinel)."""
    import torch
    sent = s.dtype(-7.25e11)
    buf = torch.full((src.size + 2 * GUARD,), float(sent), dtype=s.tdt, device=ctx.device)
    mid = buf[GUARD:GUARD + src.size]
    mid.copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
    return buf, mid, sent


def _bands_untouched(buf, sent):
    b = buf.cpu().numpy()
    return bool((_bits(b[:GUARD]) == _bits(np.array([sent]))[0]).all() and (_bits(b[-GUARD:]) == _bits(np.array([sent]))[0]).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_build_gives_the_list_of_the_definition(ctx, case):
    """fix_start, fix_off, fix_val and count equal the expected arrays exactly; the count-only form gives the same table; a
    second call gives the same bytes; the mark kernel is named."""
    n, dtype, mode, kind = case
    s = _data(ctx, n, dtype, mode, kind)
    assert s.sf == 100.0
    tn = "double" if dtype == np.float64 else "float"
    counts = []
    for m in MULTS:
        b = m * EB * s.sf
        what = f"{_id(case)} m={m}"
        want = s.expect(b)
        fix = s.build(ctx, b)
        assert ctx.last_kernel(1) == f"{'k_fixup_mark' if n >= 64 else 'k_fixup_mark_rem'}<{tn}, {mode}>"
        _same_list(fix, want, what)
        start0, off0, val0, k0 = s.build(ctx, b, capacity=0)
        assert off0 is None and val0 is None and k0 == fix[3], what
        assert np.array_equal(start0.cpu().numpy().view(np.uint32), want[1]), what
        if fix[3]:
            again = s.build(ctx, b, capacity=fix[3])
            for a_, b_ in zip(_fix_np(again)[:3], _fix_np(fix)[:3]):
                assert np.array_equal(_bits(a_), _bits(b_)), what
        counts.append(fix[3])
    print(f"{_id(case)}: listed for m = {MULTS}: {counts}")
    # neither end of the cases can go vacuous: the dense case lists more than half of some tile, the empty case nothing
    if kind == "noisy" and n >= TILE:
        per = np.diff(s.expect(MULTS[0] * EB * s.sf)[1].astype(np.int64))
        assert per.max() > TILE // 2, per
    assert counts[-1] == 0 and s.expect(MULTS[-1] * EB * s.sf)[1][-1] == 0
    assert counts[0] > 0 and counts == sorted(counts, reverse=True)
    if n % 64 == 37 and kind == "noisy":
        assert s.expect(MULTS[0] * EB * s.sf)[0][n // 64 * 64:].any()           # the short block of 37 elements has entries


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "noisy"], ids=_id)
def test_a_list_that_does_not_fit_is_counted_and_not_written(ctx, case):
    import torch
    n, dtype, mode, kind = case
    s = _data(ctx, n, dtype, mode, kind)
    b = 0.5 * EB * s.sf
    want = s.expect(b)
    k = int(want[1][-1])
    assert k >= 2
    start = torch.zeros(want[1].size, dtype=torch.int32, device=ctx.device)
    off = torch.full((k,), 0x5a5a, dtype=torch.int16, device=ctx.device)
    val = torch.full((k,), -7.25e11, dtype=s.tdt, device=ctx.device)
    off0, val0 = off.cpu().numpy().copy(), val.cpu().numpy().copy()
    count = C.c_uint32(0)
    assert s.raw_build(ctx, b, start, off, val, k - 1, count) == H.E_SPACE
    assert count.value == k
    assert np.array_equal(start.cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(off.cpu().numpy(), off0) and np.array_equal(_bits(val.cpu().numpy()), _bits(val0))
    # the same buffers with room: the list
    assert s.raw_build(ctx, b, start, off, val, k, count) == H.OK and count.value == k
    _same_list((start, off, val, k), want, _id(case))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_apply_to_the_whole_array(ctx, case):
    n, dtype, mode, kind = case
    s = _data(ctx, n, dtype, mode, kind)
    for m in MULTS:
        b = m * EB * s.sf
        fix = s.build(ctx, b)
        buf, mid, sent = _guarded(ctx, s, s.full)
        ctx.fixup_apply(fix, n, s.tdt, mid)
        assert ctx.last_kernel(1) == f"k_fixup_apply<{'double' if dtype == np.float64 else 'float'}>"
        got = mid.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(s.applied(b))), (_id(case), m)
        _guarantee(s.x, got, b, (_id(case), m))
        assert _bands_untouched(buf, sent)


@pytest.mark.parametrize("case", [(FLAT_N[-1], np.float64, H.EC, "noisy"), (FLAT_N[-1], np.float32, H.QT, "noisy"),
                                  (FLAT_N[-1], np.float64, H.QT, "smooth")], ids=_id)
def test_apply_to_a_range(ctx, case):
    """An unaligned range across two tile borders and into the short block, on decompress_range's output."""
    n, dtype, mode, kind = case
    s = _data(ctx, n, dtype, mode, kind)
    lo, hi = 4000, n - 5
    assert hi > n // 64 * 64 and lo % 64 and hi % 64
    for m in (0.25, 0.5):
        b = m * EB * s.sf
        fix = s.build(ctx, b)
        part = ctx.decompress_range(s.out, s.cnt, n, s.tdt, EB, s.sf, lo, hi, s.idx, mode=mode, qtable=s.q)
        assert np.array_equal(_bits(part.cpu().numpy()), _bits(s.full[lo:hi]))
        buf, mid, sent = _guarded(ctx, s, part.cpu().numpy())
        ctx.fixup_apply(fix, n, s.tdt, mid, lo=lo, hi=hi)
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(s.applied(b)[lo:hi])), (_id(case), m)
        assert _bands_untouched(buf, sent)
    # a range inside one tile that holds no tile border at all
    b = 0.25 * EB * s.sf
    fix = s.build(ctx, b)
    part = ctx.decompress_range(s.out, s.cnt, n, s.tdt, EB, s.sf, 4100, 4200, s.idx, mode=mode, qtable=s.q)
    ctx.fixup_apply(fix, n, s.tdt, part, lo=4100, hi=4200)
    assert np.array_equal(_bits(part.cpu().numpy()), _bits(s.applied(b)[4100:4200]))


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
def test_apply_to_boxes(ctx, dtype, mode):
    """A 2-D and a 3-D box that cut tiles, on decompress_box's output: each equals the slice of the whole-array result."""
    n = 3 * TILE
    s = _data(ctx, n, dtype, mode, "noisy")
    b = 0.5 * EB * s.sf
    fix = s.build(ctx, b)
    whole = s.applied(b)
    assert fix[3] > 1000
    for dims, lo, hi in (((12, 1024), (1, 100), (11, 900)), ((6, 8, 256), (1, 2, 10), (5, 7, 200)), ((12, 1024), (0, 0), (12, 1024)),
                         ((3, 4096), (1, 4095), (2, 4096))):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        box = ctx.decompress_box(s.out, s.cnt, dims, s.tdt, EB, s.sf, lo, hi, s.idx, mode=mode, qtable=s.q)
        assert np.array_equal(_bits(box.cpu().numpy()), _bits(s.full.reshape(dims)[sl]))
        buf, mid, sent = _guarded(ctx, s, box.cpu().numpy())
        ctx.fixup_apply(fix, n, s.tdt, mid, dims=dims, lo=lo, hi=hi)
        want = np.ascontiguousarray(whole.reshape(dims)[sl]).reshape(-1)
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(want)), (dims, lo, hi)
        assert _bands_untouched(buf, sent)


def test_more_tiles_than_resident_workgroups(ctx):
    """2052 tiles: the grid-stride loops of mark, emit and apply, and a scan of more than one level."""
    n, dtype, mode = BIG_N, np.float64, H.EC
    s = Streams(ctx, _field(n, "noisy", dtype, seed=7), mode)
    b = 0.5 * EB * s.sf
    want = s.expect(b)
    fix = s.build(ctx, b)
    _same_list(fix, want, "big")
    assert fix[3] > n // 8
    out = ctx.decompress(s.out, s.cnt, n, s.tdt, EB, s.sf, mode)
    ctx.fixup_apply(fix, n, s.tdt, out)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(s.applied(b)))
    _guarantee(s.x, got, b, "big")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_nan_lists_its_block_and_stays_a_nan(ctx, dtype):
    """tests/nonfinite.py's qnan_one: one NaN mid-array takes its block down on decode.  All 64 elements are listed; after apply
    the 63 others have x's bits and the NaN is a NaN; every other block's entries are those of the finite array."""
    n, mode = FLAT_N[-1], H.EC
    base = _field(n, "noisy", dtype, seed=n) * dtype(0.09)               # |x| < 100, as nonfinite.make asks; sf = 10
    x, bad = NF.make("qnan_one", n, dtype, base=base)
    assert bad.size == 1
    s, sb = Streams(ctx, x, mode), Streams(ctx, base, mode)
    assert s.sf == sb.sf == 10.0
    lo = 64 * int(bad[0])
    assert np.isnan(s.full[lo:lo + 64]).all() and int(np.isnan(s.full).sum()) == 64 and int(np.isnan(x).sum()) == 1
    b = 0.5 * EB * s.sf
    want = s.expect(b)
    assert want[0][lo:lo + 64].all()
    fix, fixb = s.build(ctx, b), sb.build(ctx, b)
    _same_list(fix, want, "nan")
    # outside the block: the finite array's entries
    mb = sb.expect(b)[0]
    other = np.ones(n, bool)
    other[lo:lo + 64] = False
    assert np.array_equal(want[0][other], mb[other]) and fix[3] == fixb[3] - int(mb[lo:lo + 64].sum()) + 64
    out = ctx.decompress(s.out, s.cnt, n, s.tdt, EB, s.sf, mode)
    ctx.fixup_apply(fix, n, s.tdt, out)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[lo:lo + 64]), _bits(x[lo:lo + 64])) and int(np.isnan(got).sum()) == 1
    assert np.array_equal(_bits(got), _bits(s.applied(b)))
    _guarantee(x, got, b, "nan")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_short_block_of_nans(ctx, dtype):
    """A NaN in the short last block: the block decodes to NaNs, all of it is listed and restored."""
    n, mode = FLAT_N[-1], H.EC
    base = _field(n, "smooth", dtype, seed=n) * dtype(0.09)
    x, bad = NF.make("nan_last_short", n, dtype, base=base)
    s = Streams(ctx, x, mode)
    lo = n // 64 * 64
    assert np.isnan(s.full[lo:]).all() and int(np.isnan(s.full).sum()) == n - lo
    b = 2.0 * EB * s.sf
    want = s.expect(b)
    assert want[0][lo:].all() and int(want[1][-1]) == n - lo                  # nothing else is listed at m = 2
    fix = s.build(ctx, b)
    _same_list(fix, want, "short nan")
    out = ctx.decompress(s.out, s.cnt, n, s.tdt, EB, s.sf, mode, qtable=s.q)
    ctx.fixup_apply(fix, n, s.tdt, out)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[lo:]), _bits(x[lo:])) and int(np.isnan(got).sum()) == 1
    _guarantee(x, got, b, "short nan")


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
def test_build_refusals_leave_the_context_usable(ctx, dtype, mode):
    import torch
    n = FLAT_N[-1]
    s = _data(ctx, n, dtype, mode, "noisy")
    b = 0.5 * EB * s.sf
    want = s.expect(b)
    k = int(want[1][-1])
    start = torch.zeros(want[1].size, dtype=torch.int32, device=ctx.device)
    off = torch.zeros(k, dtype=torch.int16, device=ctx.device)
    val = torch.zeros(k, dtype=s.tdt, device=ctx.device)
    count = C.c_uint32(0)

    def after():
        assert s.raw_build(ctx, b, start, off, val, k, count) == H.OK and count.value == k
        _same_list((start, off, val, k), want, "after a refusal")

    after()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert s.raw_build(ctx, bad, start, off, val, k, count) == H.E_ARG, bad
        after()
    assert s.raw_build(ctx, b, start, off, val, k, count, ref=None) == H.E_ARG
    after()
    assert s.raw_build(ctx, b, start, off, None, k, count) == H.E_ARG           # exactly one of the two list pointers
    assert s.raw_build(ctx, b, start, None, val, k, count) == H.E_ARG
    after()
    # an output over an input, and the two list arrays over each other
    assert s.raw_build(ctx, b, s.idx, off, val, k, count) == H.E_ARG
    assert s.raw_build(ctx, b, start, off, s.xd, k, count) == H.E_ARG
    after()
    # an index that disagrees with the flags: a checked refusal on the device, and the next call is clean
    ix = s.idx.clone()
    ix[2] += 1
    assert s.raw_build(ctx, b, start, off, val, k, count, idx=ix) == H.E_ARG
    after()


def _raw_apply(ctx, s, start, off, val, count, mid, lo=0, hi=None):
    arr = C.c_size_t * 1
    return ctx.lib.dctzhip_fixup_apply(ctx.h, start.data_ptr(), off.data_ptr(), val.data_ptr(), int(count), s.n, H._dt(s.tdt), 1, arr(s.n), arr(lo),
                                       arr(s.n if hi is None else hi), mid.data_ptr())


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
def test_apply_refuses_a_tampered_list(ctx, dtype, mode):
    """The list is untrusted: each tampering returns E_ARG, the sentinels around the output stay, and the next call is clean."""
    n = FLAT_N[-1]
    s = _data(ctx, n, dtype, mode, "noisy")
    b = 0.5 * EB * s.sf
    start, off, val, k = s.build(ctx, b)
    sn = start.cpu().numpy()
    assert all(sn[t + 1] - sn[t] >= 2 for t in range(sn.size - 1))

    def run(st, of, kk, lo=0, hi=None):
        src = s.full[lo:hi]
        buf, mid, sent = _guarded(ctx, s, src)
        rc = _raw_apply(ctx, s, st, of, val, kk, mid, lo, hi)
        assert _bands_untouched(buf, sent)
        return rc, mid

    def clean():
        rc, mid = run(start, off, k)
        assert rc == H.OK and np.array_equal(_bits(mid.cpu().numpy()), _bits(s.applied(b)))

    clean()
    t1 = start.clone(); t1[2] = t1[1] - 1                                      # a step made negative
    assert run(t1, off, k)[0] == H.E_ARG
    clean()
    t2 = start.clone(); t2[-1] -= 1                                            # fix_start[m] != count
    assert run(t2, off, k)[0] == H.E_ARG
    assert run(start, off, k - 1)[0] == H.E_ARG                                # ... and a count that is not the table's
    clean()
    t3 = start.clone(); t3[1] += 1; t3[2:] += 5000                             # fix_start[t + 1] > count
    assert run(t3, off, k)[0] == H.E_ARG
    clean()
    o1 = off.clone(); o1[1] = o1[0]                                            # two equal offsets
    assert run(start, o1, k)[0] == H.E_ARG
    o2 = off.clone(); o2[int(sn[1]) + 1] = o2[int(sn[1])] - 1 if int(o2[int(sn[1])]) > 0 else 0   # descending inside tile 1
    assert run(start, o2, k)[0] == H.E_ARG
    o3 = off.clone(); o3[-1] = 4095                                            # beyond the last tile's 357 elements
    assert run(start, o3, k)[0] == H.E_ARG
    clean()
    # a range apply visits its own tiles only: tampering in tile 0 does not reach a range inside tiles 1 .. 2, tampering
    # in tile 1 does
    rc, mid = run(start, o1, k, 4100, 9000)
    assert rc == H.OK and np.array_equal(_bits(mid.cpu().numpy()), _bits(s.applied(b)[4100:9000]))
    assert run(start, o2, k, 4100, 9000)[0] == H.E_ARG
    clean()
    # an offset of 4095 in a 37-element array
    s37 = _data(ctx, 37, dtype, mode, "noisy")
    b37 = 0.25 * EB * s37.sf
    st, of, va, kk = s37.build(ctx, b37)
    assert kk >= 2
    bad = of.clone(); bad[-1] = 4095
    buf, mid, sent = _guarded(ctx, s37, s37.full)
    assert _raw_apply(ctx, s37, st, bad, va, kk, mid) == H.E_ARG and _bands_untouched(buf, sent)
    assert _raw_apply(ctx, s37, st, of, va, kk, mid) == H.OK and _bands_untouched(buf, sent)
    # host-side refusals: a count beyond n, a box outside the array, null pointers
    assert _raw_apply(ctx, s, start, off, val, n + 1, mid) == H.E_ARG
    buf, mid, sent = _guarded(ctx, s, s.full)
    assert _raw_apply(ctx, s, start, off, val, k, mid, 5, n + 1) == H.E_ARG and _bands_untouched(buf, sent)
    arr = C.c_size_t * 1
    assert ctx.lib.dctzhip_fixup_apply(ctx.h, None, off.data_ptr(), val.data_ptr(), k, n, H._dt(s.tdt), 1, arr(n), arr(0), arr(n), mid.data_ptr()) == H.E_ARG
    assert ctx.lib.dctzhip_fixup_apply(ctx.h, start.data_ptr(), None, val.data_ptr(), k, n, H._dt(s.tdt), 1, arr(n), arr(0), arr(n), mid.data_ptr()) == H.E_ARG
    assert ctx.lib.dctzhip_fixup_apply(ctx.h, start.data_ptr(), off.data_ptr(), val.data_ptr(), k, n, H._dt(s.tdt), 1, arr(n), arr(0), arr(n), None) == H.E_ARG
    clean()


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_dropin_round_trip(mode):
    """dctz_compress -> dctz_fixup_build (with the unscaled copy) -> dctz_decompress_bounded: the result meets the guarantee and
    is the plain decode with the listed elements restored; without the blob dctz_decompress gives the same bytes as before."""
    lib = D._lib(mode)
    lib.dctz_fixup_build.restype = C.c_int
    lib.dctz_fixup_build.argtypes = [C.POINTER(D.TVar), C.POINTER(D.TVar), C.c_int, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.dctz_decompress_bounded.restype = C.c_int
    lib.dctz_decompress_bounded.argtypes = [C.POINTER(D.TVar), C.c_void_p, C.c_size_t, C.POINTER(D.TVar)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for dtype in (np.float64, np.float32):
        n = FLAT_N[-1]
        x = _field(n, "noisy", dtype, seed=n)
        z, full = D._container(lib, x, EB, False)
        zv = D._tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])
        bound = 0.5 * EB * 100.0
        with np.errstate(invalid="ignore"):
            mask = ~(np.abs(x - full) <= dtype(bound))
        assert 1000 < int(mask.sum()) < n
        blob, nbytes = C.c_void_p(), C.c_size_t(0)
        ref = x.copy()
        assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n, bound, C.byref(blob), C.byref(nbytes)) == 1
        try:
            raw = C.string_at(blob, nbytes.value)
            assert raw[:4] == b"DZFX"
            hdr = np.frombuffer(raw[:48], dtype=np.uint32)
            assert hdr[1] == 1 and hdr[2] == (1 if dtype == np.float64 else 0)
            hn, tiles, count = (int(v) for v in np.frombuffer(raw[16:40], dtype=np.uint64))
            assert (hn, tiles, count) == (n, -(-n // TILE), int(mask.sum()))
            assert np.frombuffer(raw[40:48], dtype=np.float64)[0] == bound
            out = np.empty_like(x)
            assert lib.dctz_decompress_bounded(C.byref(zv), blob, nbytes.value, C.byref(D._tvar(out))) == 1
            assert np.array_equal(_bits(out), _bits(np.where(mask, x, full)))
            _guarantee(x, out, bound, mode)
            # a blob for another array, and a list that contradicts itself
            assert lib.dctz_decompress_bounded(C.byref(zv), blob, nbytes.value - 8, C.byref(D._tvar(out))) == -1
            tam = bytearray(raw)
            tam[48 + 4:48 + 8] = np.array([n + 1], dtype=np.uint32).tobytes()     # fix_start[1] beyond count
            tb = (C.c_char * len(tam)).from_buffer(tam)
            assert lib.dctz_decompress_bounded(C.byref(zv), tb, len(tam), C.byref(D._tvar(out))) == -1
        finally:
            libc.free(blob)
        again = np.empty_like(x)
        assert lib.dctz_decompress(C.byref(zv), C.byref(D._tvar(again))) == 1
        assert np.array_equal(_bits(again), _bits(full))
        # refusals: a reference of another length or type, a bound that is none
        assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n - 1, bound, C.byref(blob), C.byref(nbytes)) == -1
        other = ref.astype(np.float32 if dtype == np.float64 else np.float64)
        assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(other)), n, bound, C.byref(blob), C.byref(nbytes)) == -1
        assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n, -1.0, C.byref(blob), C.byref(nbytes)) == -1
