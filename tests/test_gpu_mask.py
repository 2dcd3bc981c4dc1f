"""Missing values (include/dctz_hip.h: dctzhip_mask_build / dctzhip_mask_apply / dctzhip_compress_masked): the mask, the count
and the filled array against the numpy restatement of tests/mask_cases.py, bit for bit; the masked compress call against the
plain call on the filled array and against the CPU oracle; the apply call on the output of every decode path; and what the
layer is for: a field with 1e36 holes keeps the scaling factor of its valid data, a NaN costs one element instead of 64."""
import ctypes as C

import numpy as np
import pytest

from dctz_amd import hip as H
from oracle import oracle as O
from tests import mask_cases as M
from tests import workloads as W

pytestmark = pytest.mark.gpu

EB = 1e-3
TILE = 4096
GUARD = 64                            # sentinel elements on either side of an array (a multiple of 16 bytes in both types)
MGUARD = 8                            # sentinel words on either side of a mask
MSENT = 0x5A5A5A5A5A5A5A5A
ONE_N = 2 ** 18 + 29                  # compressed by the one-launch kernel
BIG_N = 2051 * 4096 + 100             # beyond it, and several trips of the fill's and the apply's grid-stride loops
FILL = -9.96921e36                    # netCDF's default fill for floats, as a stand-in for "the caller's fill"


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
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _sent(dtype):
    return np.dtype(dtype).type(-7.25e11)


def _guarded(ctx, dtype, n, src=None):
    """n elements between two bands of sentinels on the device (src, numpy, copied into the middle; else sentinels too)."""
    import torch
    buf = torch.full((n + 2 * GUARD,), float(_sent(dtype)), dtype=_tdt(dtype), device=ctx.device)
    mid = buf[GUARD:GUARD + n]
    if src is not None:
        mid.copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
    return buf, mid


def _bands_untouched(buf, dtype):
    b = buf.cpu().numpy()
    s = _bits(np.array([_sent(dtype)]))[0]
    return bool((_bits(b[:GUARD]) == s).all() and (_bits(b[-GUARD:]) == s).all())


def _guarded_mask(ctx, n):
    import torch
    words = -(-n // 64)
    buf = torch.full((words + 2 * MGUARD,), MSENT, dtype=torch.int64, device=ctx.device)
    return buf, buf[MGUARD:MGUARD + words]


def _mask_bands_untouched(buf):
    b = buf.cpu().numpy().view(np.uint64)
    return bool((b[:MGUARD] == MSENT).all() and (b[-MGUARD:] == MSENT).all())


def _words(mask):
    return mask.cpu().numpy().view(np.uint64)


# ---- build: mask, count, filled array ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("n", M.SIZES)
def test_build_equals_the_restatement(ctx, dtype, n):
    """Every pattern under every rule: mask words, count and filled array are the restatement's, bit for bit; the input is
    unchanged; a second call gives the same bytes; in place equals out of place; without a filled array the mask and the
    count are the same and nothing else is written; the bands around every output stay."""
    tn = "double" if dtype == np.float64 else "float"
    for rule, (flags, value, limit) in M.RULES.items():
        for pat in M.PATTERNS:
            what = (rule, pat)
            x, miss = M.build_input(n, dtype, pat, rule)
            assert np.array_equal(M.is_missing(x, flags, value, limit), miss), what
            want_w, want_f, want_c = M.mask_words(miss), M.fill(x, miss), int(miss.sum())
            xd = _dev(ctx, x)
            fbuf, fmid = _guarded(ctx, dtype, n)
            mbuf, mmid = _guarded_mask(ctx, n)
            mask, count, filled = ctx.mask_build(xd, flags, value, limit, filled=fmid, mask=mmid)
            assert ctx.last_kernel(1) == f"k_mask_fill<{tn}>"
            assert count == want_c, what
            assert np.array_equal(_words(mask), want_w), what
            assert np.array_equal(_bits(filled.cpu().numpy()), _bits(want_f)), what
            assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), what
            assert _bands_untouched(fbuf, dtype) and _mask_bands_untouched(mbuf), what
            # again, into buffers that hold other bytes
            fbuf2, fmid2 = _guarded(ctx, dtype, n, src=np.zeros(n, dtype))
            mbuf2, mmid2 = _guarded_mask(ctx, n)
            mmid2.zero_()
            _, count2, _ = ctx.mask_build(xd, flags, value, limit, filled=fmid2, mask=mmid2)
            assert count2 == count and np.array_equal(_words(mmid2), _words(mask)), what
            assert np.array_equal(_bits(fmid2.cpu().numpy()), _bits(filled.cpu().numpy())), what
            # mask and count only
            mbuf3, mmid3 = _guarded_mask(ctx, n)
            _, count3, none = ctx.mask_build(xd, flags, value, limit, filled=False, mask=mmid3)
            assert none is None and count3 == want_c and np.array_equal(_words(mmid3), want_w), what
            assert _mask_bands_untouched(mbuf3) and np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), what
            # in place
            ibuf, imid = _guarded(ctx, dtype, n, src=x)
            mbuf4, mmid4 = _guarded_mask(ctx, n)
            _, count4, same = ctx.mask_build(imid, flags, value, limit, filled=imid, mask=mmid4)
            assert same is imid and count4 == want_c and np.array_equal(_words(mmid4), want_w), what
            assert np.array_equal(_bits(imid.cpu().numpy()), _bits(want_f)), what
            assert _bands_untouched(ibuf, dtype) and _mask_bands_untouched(mbuf4), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_special_values(ctx, dtype):
    """-0.0 against value = 0, infinities, a signalling NaN and denormals, each on the valid and on the missing side."""
    T = np.dtype(dtype).type
    tiny = np.finfo(dtype).tiny
    snan = M.markers("nan", dtype)[1:2]
    x = np.array([1.5, -0.0, 0.0, tiny / 8, np.inf, -np.inf, 2.5, 0.0, 3.5], dtype)
    x = np.concatenate([x, snan, np.array([4.5], dtype)])
    xd = _dev(ctx, x)
    # value = 0: both zeros are missing, the denormal is not (no flush to zero), the NaN and the infinities stay as they are
    mask, count, filled = ctx.mask_build(xd, H.MISS_VALUE, value=0.0)
    miss = np.zeros(x.size, bool)
    miss[[1, 2, 7]] = True
    assert count == 3 and np.array_equal(_words(mask), M.mask_words(miss))
    assert np.array_equal(_bits(filled.cpu().numpy()), _bits(M.fill(x, miss)))
    assert _bits(filled.cpu().numpy())[9] == _bits(snan)[0]                      # the signalling NaN kept its bits
    # value = a denormal matches exactly that denormal
    mask, count, _ = ctx.mask_build(xd, H.MISS_VALUE, value=float(T(tiny / 8)))
    assert count == 1 and int(_words(mask)[0]) == 1 << 3
    # NaN: the signalling NaN is missing; INF: both infinities; ABS_GE with a denormal limit: everything but the zeros and NaN
    assert int(_words(ctx.mask_build(xd, H.MISS_NAN)[0])[0]) == 1 << 9
    assert int(_words(ctx.mask_build(xd, H.MISS_INF)[0])[0]) == (1 << 4) | (1 << 5)
    got = int(_words(ctx.mask_build(xd, H.MISS_ABS_GE, limit=float(T(tiny / 8)))[0])[0])
    assert got == 0b10101111001
    mask, count, filled = ctx.mask_build(xd, H.MISS_NAN | H.MISS_INF | H.MISS_ABS_GE, limit=4.0)
    miss = M.is_missing(x, 11, 0.0, 4.0)
    assert miss.nonzero()[0].tolist() == [4, 5, 9, 10] and np.array_equal(_words(mask), M.mask_words(miss))
    assert np.array_equal(_bits(filled.cpu().numpy()), _bits(M.fill(x, miss)))


def test_build_refusals_leave_the_context_usable(ctx):
    """Each refusal of the contract is DCTZHIP_E_ARG before any launch: the sentinels in every buffer stay."""
    import torch
    n = 4097
    x = M.smooth(n, np.float64)
    xd = _dev(ctx, x)
    fbuf, fmid = _guarded(ctx, np.float64, n)
    mbuf, mmid = _guarded_mask(ctx, n)
    count = C.c_uint64(77)
    lib, good = ctx.lib, H.Missing(H.MISS_NAN, 0.0, 0.0)

    def call(d_in=xd.data_ptr(), n_=n, dt=H.F64, miss=good, mask=mmid.data_ptr(), filled=fmid.data_ptr(), cnt=count):
        return lib.dctzhip_mask_build(ctx.h, d_in, n_, dt, C.byref(miss) if miss is not None else None, mask, filled,
                                      C.byref(cnt) if cnt is not None else None)

    assert lib.dctzhip_mask_build(None, xd.data_ptr(), n, H.F64, C.byref(good), mmid.data_ptr(), fmid.data_ptr(), C.byref(count)) == H.E_ARG
    for kw in (dict(d_in=None), dict(miss=None), dict(mask=None), dict(cnt=None), dict(n_=0), dict(dt=2), dict(dt=-1),
               dict(miss=H.Missing(0, 0.0, 0.0)), dict(miss=H.Missing(16, 0.0, 0.0)), dict(miss=H.Missing(H.MISS_NAN | 32, 0.0, 0.0)),
               dict(miss=H.Missing(H.MISS_VALUE, float("nan"), 0.0)),
               dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, 0.0)), dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, -1.0)),
               dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, float("inf"))), dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, float("nan"))),
               dict(d_in=xd.data_ptr() + 8), dict(filled=fmid.data_ptr() + 8), dict(mask=mmid.data_ptr() + 4),
               dict(filled=xd.data_ptr() + 16),                                    # a partial overlap of the filled copy and the input
               dict(filled=xd.data_ptr() + 8 * (n - 1) - 7),                       # ... by its last element alone (and misaligned)
               dict(filled=xd.data_ptr() + 1600),
               dict(mask=xd.data_ptr() + 64), dict(mask=fmid.data_ptr() + 64)):   # the mask inside an array
        assert call(**kw) == H.E_ARG, kw
        assert ctx.lib.dctzhip_last_error(ctx.h)
    assert count.value == 77
    assert _bands_untouched(fbuf, np.float64) and _mask_bands_untouched(mbuf)
    s = _bits(np.array([_sent(np.float64)]))[0]
    assert (_bits(fmid.cpu().numpy()) == s).all() and (_words(mmid) == MSENT).all()
    # a NaN value or a bad limit is only looked at when its test is selected
    assert call(miss=H.Missing(H.MISS_NAN, float("nan"), -1.0)) == H.OK and count.value == 0
    # compress_masked: its own refusals, and the filled copy may not be the input
    out = ctx.alloc_outputs(n, torch.float64)
    info = H.CompressInfo()

    def cm(d_in=xd.data_ptr(), eb=EB, mode=H.EC, miss=good, b=out["bin_index"].data_ptr(), mask=mmid.data_ptr(), filled=fmid.data_ptr()):
        return lib.dctzhip_compress_masked(ctx.h, d_in, n, H.F64, eb, mode, C.byref(miss) if miss is not None else None, b,
                                           out["dc"].data_ptr(), out["ac_exact"].data_ptr(), mask, filled, C.byref(info), C.byref(count))

    fmid.fill_(float(_sent(np.float64)))
    for kw in (dict(d_in=None), dict(miss=None), dict(b=None), dict(mask=None), dict(mode=2), dict(miss=H.Missing(0, 0.0, 0.0)),
               dict(filled=xd.data_ptr()), dict(filled=xd.data_ptr() + 16), dict(mask=out["bin_index"].data_ptr()),
               dict(b=out["bin_index"].data_ptr() + 8), dict(mask=mmid.data_ptr() + 4)):
        assert cm(**kw) == H.E_ARG, kw
    assert cm(eb=1e-7) == H.E_BOUND
    assert (_bits(fmid.cpu().numpy()) == s).all()
    assert cm() == H.OK and info.sf == 1.0


# ---- compress_masked ----------------------------------------------------------------------------------------------------
def _holey(n, dtype):
    """Finite data with 1e36 in blobs."""
    x = W.ragged(n, dtype)
    miss = M.pattern("blobs", n)
    x[miss] = 1e36
    return x, miss


def _same_streams(out, info, ref_out, ref_info, what):
    import torch
    assert info.cnt == ref_info.cnt and info.nblk == ref_info.nblk, what
    # (flags name the route a call took through the library, which follows what the context ran before: not compared)
    for f in ("sf", "mean", "max_abs", "min_abs"):
        assert np.float64(getattr(info, f)).view(np.uint64) == np.float64(getattr(ref_info, f)).view(np.uint64), (what, f)
    assert list(info.qtable) == list(ref_info.qtable) and list(info.qtable_raw) == list(ref_info.qtable_raw), what
    assert torch.equal(out["bin_index"], ref_out["bin_index"]), what
    assert torch.equal(out["dc"].view(torch.int32), ref_out["dc"].view(torch.int32)), what
    assert torch.equal(out["ac_exact"][:info.cnt].view(torch.int32), ref_out["ac_exact"][:info.cnt].view(torch.int32)), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("n", [ONE_N, BIG_N])
def test_compress_masked_is_compress_of_the_filled_array(ctx, dtype, mode, n):
    x, miss = _holey(n, dtype)
    want_f = M.fill(x, miss)
    xd = _dev(ctx, x)
    fbuf, fmid = _guarded(ctx, dtype, n)
    mbuf, mmid = _guarded_mask(ctx, n)
    out, info, mask, count = ctx.compress_masked(xd, EB, H.MISS_VALUE, value=1e36, mode=mode, filled=fmid, mask=mmid)
    assert count == int(miss.sum()) and np.array_equal(_words(mask), M.mask_words(miss))
    assert np.array_equal(_bits(fmid.cpu().numpy()), _bits(want_f))
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), "d_in is not modified"
    assert _bands_untouched(fbuf, dtype) and _mask_bands_untouched(mbuf)
    ref_out, ref_info = ctx.compress(_dev(ctx, want_f), EB, mode)
    assert bool(ref_info.flags & H.INFO_ONE_LAUNCH) == (n == ONE_N)               # a size on each side of the one-launch limit
    assert bool(info.flags & H.INFO_ONE_LAUNCH) == (n == ONE_N)
    _same_streams(out, info, ref_out, ref_info, "against ctx.compress")
    # the filled copy kept by the context
    out2, info2, mask2, count2 = ctx.compress_masked(xd, EB, H.MISS_VALUE, value=1e36, mode=mode)
    assert count2 == count and np.array_equal(_words(mask2), _words(mask))
    _same_streams(out2, info2, ref_out, ref_info, "context scratch")
    c = O.compress(want_f, EB, mode, O.FAST)
    assert info.sf == c.sf and info.cnt == c.cnt
    assert np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)
    assert np.array_equal(_bits(out["dc"].cpu().numpy()), _bits(c.dc))
    assert np.array_equal(_bits(out["ac_exact"][:c.cnt].cpu().numpy()), _bits(c.ac_exact))
    if mode == H.QT:
        assert np.array_equal(_bits(np.array(info.qtable[:], dtype=dtype)), _bits(c.qtable))
    # the whole-array apply on this size: several trips of its loop
    q = np.array(info.qtable[:]) if mode == H.QT else None
    dec = ctx.decompress(out, info.cnt, n, _tdt(dtype), EB, info.sf, mode, qtable=q)
    before = dec.cpu().numpy()
    ctx.mask_apply(mask, n, FILL, dec)
    assert np.array_equal(_bits(dec.cpu().numpy()), _bits(np.where(miss, dtype(FILL), before)))


# ---- apply --------------------------------------------------------------------------------------------------------------
class Masked:
    """One holey array on the device: mask, filled copy, streams of the filled copy, index, full decode."""

    def __init__(self, ctx, x, flags, value, limit, mode):
        self.x, self.n, self.mode, self.dtype = x, x.size, mode, x.dtype.type
        self.tdt = _tdt(x.dtype)
        self.miss = M.is_missing(x, flags, value, limit)
        self.xd = _dev(ctx, x)
        self.filled = ctx.torch.empty_like(self.xd)
        self.out, self.info, self.mask, self.count = ctx.compress_masked(self.xd, EB, flags, value, limit, mode=mode, filled=self.filled)
        self.q = np.array(self.info.qtable[:]) if mode == H.QT else None
        self.sf, self.cnt = self.info.sf, self.info.cnt
        self.full = ctx.decompress(self.out, self.cnt, self.n, self.tdt, EB, self.sf, mode, qtable=self.q).cpu().numpy()
        self.idx, tot = ctx.ac_index(self.out, self.n)
        assert tot == self.cnt and self.count == int(self.miss.sum())


_DATA = {}


def _masked(ctx, n, dtype, mode):
    key = (n, np.dtype(dtype).name, mode)
    if key not in _DATA:
        x = W.ragged(n, dtype)
        miss = M.pattern("random30", n) | M.pattern("across_boundaries", n) | M.pattern("last_block_leading", n)
        x[miss] = 1e36
        _DATA[key] = Masked(ctx, x, H.MISS_VALUE, 1e36, 0.0, mode)
    return _DATA[key]


FLAT_N = 3 * TILE + 5 * 64 + 37


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT), (np.float32, H.EC)], ids=["float64-EC", "float32-QT", "float32-EC"])
def test_apply_to_whole_and_range(ctx, dtype, mode):
    n = FLAT_N
    s = _masked(ctx, n, dtype, mode)
    tn = "double" if dtype == np.float64 else "float"
    for fill in (FILL, float("nan"), 0.0):
        buf, mid = _guarded(ctx, dtype, n, src=s.full)
        ctx.mask_apply(s.mask, n, fill, mid)
        assert ctx.last_kernel(1) == f"k_mask_apply<{tn}>"
        got = mid.cpu().numpy()
        if fill != fill:                                  # a quiet NaN, its payload not pinned
            assert np.isnan(got[s.miss]).all() and np.array_equal(_bits(got[~s.miss]), _bits(s.full[~s.miss]))
        else:
            assert np.array_equal(_bits(got), _bits(np.where(s.miss, dtype(fill), s.full)))
        assert _bands_untouched(buf, dtype)
    # an unaligned range across two tile borders and into the short block, one inside a tile, one element, the last element
    for lo, hi in ((4000, n - 5), (4100, 4200), (4095, 4096), (n - 1, n), (0, 1), (63, 129)):
        part = ctx.decompress_range(s.out, s.cnt, n, s.tdt, EB, s.sf, lo, hi, s.idx, mode=mode, qtable=s.q)
        assert np.array_equal(_bits(part.cpu().numpy()), _bits(s.full[lo:hi]))
        buf, mid = _guarded(ctx, dtype, hi - lo, src=part.cpu().numpy())
        ctx.mask_apply(s.mask, n, FILL, mid, lo=lo, hi=hi)
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(np.where(s.miss[lo:hi], dtype(FILL), s.full[lo:hi]))), (lo, hi)
        assert _bands_untouched(buf, dtype)


BOXES = (((12, 1024), (1, 100), (11, 900)), ((6, 8, 256), (1, 2, 10), (5, 7, 200)), ((12, 1024), (0, 0), (12, 1024)),
         ((3, 4096), (1, 4095), (2, 4096)), ((96, 128), (5, 3), (90, 4)), ((2, 3, 8, 256), (0, 1, 2, 3), (2, 3, 7, 250)))


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
def test_apply_to_boxes(ctx, dtype, mode):
    """2-D, 3-D and 4-D boxes that cut blocks and tiles, on the output of decompress_box and of decompress_boxes."""
    n = 3 * TILE
    s = _masked(ctx, n, dtype, mode)
    for dims, lo, hi in BOXES:
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        box = ctx.decompress_box(s.out, s.cnt, dims, s.tdt, EB, s.sf, lo, hi, s.idx, mode=mode, qtable=s.q)
        dec = box.cpu().numpy()
        assert np.array_equal(_bits(dec), _bits(s.full.reshape(dims)[sl]))
        buf, mid = _guarded(ctx, dtype, dec.size, src=dec)
        ctx.mask_apply(s.mask, n, FILL, mid, dims=dims, lo=lo, hi=hi)
        want = np.where(s.miss.reshape(dims)[sl], dtype(FILL), dec).reshape(-1)
        assert np.array_equal(_bits(mid.cpu().numpy()), _bits(want)), (dims, lo, hi)
        assert _bands_untouched(buf, dtype)
    dims = (12, 1024)
    boxes = [((1, 100), (11, 900)), ((0, 0), (3, 64)), ((5, 1000), (12, 1024))]
    outs = ctx.decompress_boxes(s.out, s.cnt, dims, s.tdt, EB, s.sf, boxes, s.idx, mode=mode, qtable=s.q)
    for (lo, hi), o in zip(boxes, outs):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        dec = o.cpu().numpy()
        assert np.array_equal(_bits(dec), _bits(s.full.reshape(dims)[sl]))
        flat = o.reshape(-1)
        ctx.mask_apply(s.mask, n, FILL, flat, dims=dims, lo=lo, hi=hi)
        assert np.array_equal(_bits(flat.cpu().numpy()), _bits(np.where(s.miss.reshape(dims)[sl], dtype(FILL), dec).reshape(-1))), (lo, hi)


def test_apply_ignores_bits_beyond_n_and_takes_any_mask(ctx):
    """A mask whose tail bits beyond n are set writes nothing beyond n; an all-ones mask fills everything, and only that."""
    import torch
    for dtype in (np.float32, np.float64):
        for n in (1, 37, 65, FLAT_N):
            words = -(-n // 64)
            ones = torch.full((words,), -1, dtype=torch.int64, device=ctx.device)
            buf, mid = _guarded(ctx, dtype, n, src=M.smooth(n, dtype))
            ctx.mask_apply(ones, n, 2.5, mid)
            assert (mid.cpu().numpy() == 2.5).all() and _bands_untouched(buf, dtype), (dtype, n)
            tail = torch.zeros(words, dtype=torch.int64, device=ctx.device)
            if n % 64:
                tail[-1] = -1 << (n % 64)                 # only bits at positions >= n
                src = M.smooth(n, dtype)
                buf, mid = _guarded(ctx, dtype, n, src=src)
                ctx.mask_apply(tail, n, 2.5, mid)
                assert np.array_equal(_bits(mid.cpu().numpy()), _bits(src)) and _bands_untouched(buf, dtype), (dtype, n)


def test_apply_refusals(ctx):
    import torch
    n = 3 * TILE
    mask = torch.zeros(n // 64, dtype=torch.int64, device=ctx.device)
    out = torch.zeros(n, dtype=torch.float64, device=ctx.device)
    arr = lambda *v: (C.c_size_t * len(v))(*v)
    lib = ctx.lib

    def call(m=mask.data_ptr(), n_=n, dt=H.F64, nd=2, dims=arr(12, 1024), lo=arr(1, 100), hi=arr(11, 900), o=out.data_ptr(), h=ctx.h):
        return lib.dctzhip_mask_apply(h, m, n_, dt, 1.0, nd, dims, lo, hi, o)

    assert call() == H.OK
    for kw in (dict(h=None), dict(m=None), dict(o=None), dict(n_=0), dict(dt=3), dict(nd=0), dict(nd=5), dict(dims=None), dict(lo=None),
               dict(hi=None), dict(dims=arr(12, 1000)), dict(hi=arr(13, 900)), dict(lo=arr(11, 100)), dict(lo=arr(1, 900)),
               dict(m=mask.data_ptr() + 4), dict(o=out.data_ptr() + 4), dict(o=mask.data_ptr())):
        assert call(**kw) == H.E_ARG, kw
    assert not out.any() and call() == H.OK


# ---- what the layer is for ------------------------------------------------------------------------------------------------
def test_a_field_with_1e36_holes_keeps_the_scaling_factor_of_its_valid_data(ctx):
    """A 512 x 2048 fp32 window of workloads.c2(), about 27 % of it 1e36 in smooth blobs: the plain call scales by 1e35, the
    masked call by the sf of the valid data; after decode and apply the valid elements are bit for bit the decode of the filled
    array and the missing ones hold the fill."""
    import torch
    f = W.c2().reshape(1800, 3600)[:512, :2048].copy()
    yy, xx = np.meshgrid(np.arange(512.0), np.arange(2048.0), indexing="ij")
    miss = (np.sin(xx / 97.0 + 0.5) * np.cos(yy / 61.0) + 0.6 * np.sin((xx + 2 * yy) / 173.0)) > 0.33
    assert 0.22 < miss.mean() < 0.32, miss.mean()
    x = f.copy()
    x[miss] = 1e36
    x, miss, n = x.ravel(), miss.ravel(), f.size
    xd = _dev(ctx, x)
    _, plain = ctx.compress(xd, EB, H.EC)
    assert plain.sf == O.stats(x).sf == float(np.float32(1e35))      # (1e35 in the data's type)
    filled = torch.empty_like(xd)
    out, info, mask, count = ctx.compress_masked(xd, EB, H.MISS_VALUE, value=1e36, filled=filled)
    assert count == int(miss.sum())
    assert info.sf == O.stats(x[~miss]).sf == 1.0
    want_f = M.fill(x, miss)
    # (blocks that lie inside a blob hold +0.0: the smallest magnitude is theirs)
    assert info.max_abs == float(np.abs(x[~miss]).max()) and info.min_abs == float(np.abs(want_f).min())
    assert np.array_equal(_bits(filled.cpu().numpy()), _bits(want_f))
    dec_filled = ctx.decompress(out, info.cnt, n, torch.float32, EB, info.sf, H.EC).cpu().numpy()
    c = O.compress(want_f, EB, H.EC, O.FAST)
    assert np.array_equal(_bits(dec_filled), _bits(O.decompress(c, O.FAST)))
    dec = _dev(ctx, dec_filled)
    ctx.mask_apply(mask, n, FILL, dec)
    got = dec.cpu().numpy()
    assert np.array_equal(_bits(got[~miss]), _bits(dec_filled[~miss]))
    assert (_bits(got[miss]) == _bits(np.array([FILL], np.float32))[0]).all()
    err = np.abs(got[~miss].astype(np.float64) - x[~miss]).max()
    print(f"1e36 window: count {count}, sf plain {plain.sf:g} masked {info.sf:g}, cnt {info.cnt}, max error on valid elements {err:.3g}")
    # every coefficient of a block lies within eb sf of its original, so the block's error has an L2 norm of at most
    # sqrt(64) eb sf and no element can be further off than that (plus fp32 rounding of values below 2); the plain path's error
    # is about 1e32, every valid element being quantised against 1e35
    assert err <= 8 * EB * info.sf + 1e-5


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_a_nan_costs_one_element_not_its_block(ctx, dtype):
    """Scattered NaNs under MISS_NAN: only those elements end as the fill; the plain path loses 64 elements per NaN."""
    n = FLAT_N
    x = W.ragged(n, dtype)
    at = np.array([5, 700, 701, 4095, 4096 + 64 * 3 + 63, 9000, n - 3])
    x[at] = np.nan
    blocks = np.unique(at // 64)
    xd = _dev(ctx, x)
    tdt = _tdt(dtype)
    out0, info0 = ctx.compress(xd, EB, H.EC)
    plain = ctx.decompress(out0, info0.cnt, n, tdt, EB, info0.sf, H.EC).cpu().numpy()
    lost = np.isnan(plain)
    want_lost = np.zeros(n, bool)
    for b in blocks:
        want_lost[b * 64:(b + 1) * 64] = True
    assert np.array_equal(lost, want_lost) and lost.sum() == sum(min(64, n - b * 64) for b in blocks) > 5 * 64
    out, info, mask, count = ctx.compress_masked(xd, EB, H.MISS_NAN)
    assert count == at.size
    dec = ctx.decompress(out, info.cnt, n, tdt, EB, info.sf, H.EC)
    assert not np.isnan(dec.cpu().numpy()).any()
    ctx.mask_apply(mask, n, float("nan"), dec)
    got = dec.cpu().numpy()
    assert np.array_equal(np.flatnonzero(np.isnan(got)), at)
    ok = ~np.isnan(x)
    assert np.abs(got[ok].astype(np.float64) - x[ok]).max() <= 8 * EB * info.sf + 1e-5      # (sqrt(64) eb sf, as above)


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
def test_composed_guarantee(ctx, dtype, mode):
    """The correction list built against the FILLED array, a decode by the whole, a range and a box path, fixup_apply, then
    mask_apply: every valid element has the original's bits or lies within the bound, every missing element the fill's bits."""
    n = FLAT_N
    s = _masked(ctx, n, dtype, mode)
    bound = 0.5 * EB * s.sf
    fix = ctx.fixup_build(s.out, s.cnt, n, s.tdt, EB, s.sf, s.filled, bound, index=s.idx, mode=mode, qtable=s.q)
    listed = fix[3]
    assert listed > 0
    fillbits = _bits(np.array([FILL], dtype))[0]

    def check(got, sel, what):
        x, miss = s.x.reshape(-1)[sel], s.miss.reshape(-1)[sel]
        same = _bits(got) == _bits(x)
        with np.errstate(invalid="ignore", over="ignore"):
            near = np.abs(x - got) <= dtype(bound)
        assert bool((same | near)[~miss].all()), what
        assert bool((_bits(got)[miss] == fillbits).all()), what
        assert miss.any() and (~miss).any(), what

    whole = ctx.decompress(s.out, s.cnt, n, s.tdt, EB, s.sf, mode, qtable=s.q)
    ctx.fixup_apply(fix, n, s.tdt, whole)
    ctx.mask_apply(s.mask, n, FILL, whole)
    check(whole.cpu().numpy(), slice(None), "whole")
    lo, hi = 4000, n - 5
    part = ctx.decompress_range(s.out, s.cnt, n, s.tdt, EB, s.sf, lo, hi, s.idx, mode=mode, qtable=s.q)
    ctx.fixup_apply(fix, n, s.tdt, part, lo=lo, hi=hi)
    ctx.mask_apply(s.mask, n, FILL, part, lo=lo, hi=hi)
    check(part.cpu().numpy(), slice(lo, hi), "range")
    s3 = _masked(ctx, 3 * TILE, dtype, mode)
    fix3 = ctx.fixup_build(s3.out, s3.cnt, s3.n, s3.tdt, EB, s3.sf, s3.filled, bound, index=s3.idx, mode=mode, qtable=s3.q)
    dims, blo, bhi = (6, 8, 256), (1, 2, 10), (5, 7, 200)
    box = ctx.decompress_box(s3.out, s3.cnt, dims, s3.tdt, EB, s3.sf, blo, bhi, s3.idx, mode=mode, qtable=s3.q).reshape(-1)
    ctx.fixup_apply(fix3, s3.n, s3.tdt, box, dims=dims, lo=blo, hi=bhi)
    ctx.mask_apply(s3.mask, s3.n, FILL, box, dims=dims, lo=blo, hi=bhi)
    sl = tuple(slice(l, h) for l, h in zip(blo, bhi))
    got = box.cpu().numpy()
    x3, m3 = s3.x.reshape(dims)[sl].reshape(-1), s3.miss.reshape(dims)[sl].reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (_bits(got) == _bits(x3)) | (np.abs(x3 - got) <= dtype(bound))
    assert bool(ok[~m3].all()) and bool((_bits(got)[m3] == fillbits).all()) and m3.any()
