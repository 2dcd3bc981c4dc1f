"""Missing values of arrays compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h: dctzhip_mask_build_nd /
dctzhip_compress_masked_nd): the mask, the count and the filled array against the numpy restatement of tests/ndmask_cases.py,
bit for bit, the mask against the flat build's of the same buffer; the masked compress call against compress_nd of the filled
array; and what the layer is for: a tiled field with 1e36 holes keeps the scaling factor of its valid data, a NaN costs one
element instead of its tile, and the composed sequence -- correction list against the filled array, whole or box decode, the
list, the mask -- leaves every valid element exact or within the bound and every missing one with the fill's bits."""
import ctypes as C

import numpy as np
import pytest

from dctz_amd import hip as H
from oracle import oracle as O
from tests import mask_cases as M
from tests import ndmask_cases as N

pytestmark = pytest.mark.gpu

EB = 1e-3
GUARD = 64                            # sentinel elements on either side of an array (a multiple of 16 bytes in both types)
MGUARD = 8                            # sentinel words on either side of a mask
MSENT = 0x5A5A5A5A5A5A5A5A
FILL = -9.96921e36                    # netCDF's default fill for floats, as a stand-in for "the caller's fill"
GEOM = {2: 1, 3: 2}                   # GEOM_2D, GEOM_3D (dct_nd_block.h)


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _tn(dtype):
    return "double" if np.dtype(dtype) == np.float64 else "float"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _sent(dtype):
    return np.dtype(dtype).type(-7.25e11)


def _guarded(ctx, dtype, shape, src=None):
    """An array of `shape` between two bands of sentinels on the device (src, numpy, copied into it; else sentinels too)."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float(_sent(dtype)), dtype=_tdt(dtype), device=ctx.device)
    mid = buf[GUARD:GUARD + n].view(*shape)
    if src is not None:
        mid.copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(shape)))
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


def _build_all_ways(ctx, x, miss, flags, value, limit, what):
    """Out of place, again into buffers that hold other bytes, mask only and in place: mask words, count and filled array are the
    restatement's, bit for bit; the input is unchanged; the bands around every output stay."""
    dtype, shape, n = x.dtype.type, x.shape, x.size
    want_w, want_f, want_c = N.mask_words(miss), N.fill(x, miss), int(miss.sum())
    xd = _dev(ctx, x)
    fbuf, fmid = _guarded(ctx, dtype, shape)
    mbuf, mmid = _guarded_mask(ctx, n)
    mask, count, filled = ctx.mask_build_nd(xd, flags, value, limit, filled=fmid, mask=mmid)
    assert ctx.last_kernel(1) == f"k_ndmask_fill<{_tn(dtype)}, {GEOM[x.ndim]}>"
    assert count == want_c, what
    assert np.array_equal(_words(mask), want_w), what
    assert np.array_equal(_bits(filled.cpu().numpy()), _bits(want_f)), what
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), what
    assert _bands_untouched(fbuf, dtype) and _mask_bands_untouched(mbuf), what
    # again, into buffers that hold other bytes (a mask of ones: whatever is ORed in must have been cleared first)
    fbuf2, fmid2 = _guarded(ctx, dtype, shape, src=np.zeros(shape, dtype))
    mbuf2, mmid2 = _guarded_mask(ctx, n)
    mmid2.fill_(-1)
    _, count2, _ = ctx.mask_build_nd(xd, flags, value, limit, filled=fmid2, mask=mmid2)
    assert count2 == want_c and np.array_equal(_words(mmid2), want_w), what
    assert np.array_equal(_bits(fmid2.cpu().numpy()), _bits(want_f)), what
    assert _bands_untouched(fbuf2, dtype) and _mask_bands_untouched(mbuf2), what
    # mask and count only
    mbuf3, mmid3 = _guarded_mask(ctx, n)
    _, count3, none = ctx.mask_build_nd(xd, flags, value, limit, filled=False, mask=mmid3)
    assert none is None and count3 == want_c and np.array_equal(_words(mmid3), want_w), what
    assert _mask_bands_untouched(mbuf3) and np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), what
    # in place
    ibuf, imid = _guarded(ctx, dtype, shape, src=x)
    mbuf4, mmid4 = _guarded_mask(ctx, n)
    _, count4, same = ctx.mask_build_nd(imid, flags, value, limit, filled=imid, mask=mmid4)
    assert same is imid and count4 == want_c and np.array_equal(_words(mmid4), want_w), what
    assert np.array_equal(_bits(imid.cpu().numpy()), _bits(want_f)), what
    assert _bands_untouched(ibuf, dtype) and _mask_bands_untouched(mbuf4), what
    # byte for byte the flat layer's mask of the same buffer
    fm, fc, _ = ctx.mask_build(xd.view(-1), flags, value, limit, filled=False)
    assert fc == want_c and np.array_equal(_words(fm), want_w), what


# ---- build: mask, count, filled array ------------------------------------------------------------------------------------
def _shape_params():
    for dtype in (np.float32, np.float64):
        for shape in N.shapes(dtype):
            yield pytest.param(dtype, shape, id=f"{np.dtype(dtype).name}-{'x'.join(map(str, shape))}")


@pytest.mark.parametrize("dtype,shape", list(_shape_params()))
def test_build_equals_the_restatement(ctx, dtype, shape):
    """Every pattern under every rule."""
    for rule, (flags, value, limit) in M.RULES.items():
        for pat in N.PATTERNS:
            x, miss = N.build_input(shape, dtype, pat, rule)
            assert np.array_equal(M.is_missing(x, flags, value, limit), miss), (rule, pat)
            _build_all_ways(ctx, x, miss, flags, value, limit, (rule, pat))


@pytest.mark.parametrize("shape,dtype", N.BIG, ids=["2-D", "3-D"])
def test_build_beyond_one_trip_of_the_grid(ctx, shape, dtype):
    """Over 32 MiB: more workgroups' worth of trips than num_cu * 8, every extent ragged; 1e36 in blobs, and a NaN rule on the
    same array (nothing missing)."""
    x = N.field(shape, dtype)
    miss = N.blobs(shape)
    x[miss] = 1e36
    # a workgroup takes 16 trips of E = 16 / sizeof(T) tiles (fewer trips than this where the last one of a tile row is short)
    wgs = ctx.nd_blocks(shape) // (16 // x.itemsize) // 16
    assert x.nbytes > 32 << 20 and wgs > 8 * ctx.torch.cuda.get_device_properties(ctx.device).multi_processor_count
    _build_all_ways(ctx, x, miss, H.MISS_VALUE, 1e36, 0.0, "blobs")
    mask, count, filled = ctx.mask_build_nd(_dev(ctx, x), H.MISS_NAN)
    assert count == 0 and not _words(mask).any() and np.array_equal(_bits(filled.cpu().numpy()), _bits(x))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [(3, 4), (2, 2, 3), (2, 6)], ids=["3x4", "2x2x3", "2x6"])
def test_special_values(ctx, dtype, shape):
    """-0.0 against value = 0, infinities, a signalling NaN and a denormal, each on the valid and on the missing side."""
    tiny = np.finfo(dtype).tiny
    snan = M.markers("nan", dtype)[1:2]
    x = np.concatenate([np.array([0.0, 1.5, -0.0, tiny / 8, np.inf, -np.inf, 2.5, 0.0, 3.5], dtype), snan, np.array([4.5, -0.0], dtype)])
    x = x.reshape(shape)
    xd = _dev(ctx, x)
    # value = 0: every zero of either sign is missing, the denormal is not; the NaN and the infinities stay as they are
    mask, count, filled = ctx.mask_build_nd(xd, H.MISS_VALUE, value=0.0)
    miss = np.zeros(12, bool)
    miss[[0, 2, 7, 11]] = True
    miss = miss.reshape(shape)
    got = filled.cpu().numpy()
    assert count == 4 and np.array_equal(_words(mask), N.mask_words(miss))
    assert np.array_equal(_bits(got), _bits(N.fill(x, miss)))
    assert _bits(got).reshape(-1)[9] == _bits(snan)[0]                       # the signalling NaN kept its bits
    assert _bits(got).reshape(-1)[0] == _bits(x).reshape(-1)[1]              # the leading gap took the tile's first valid value
    for flags, limit in ((H.MISS_NAN, 0.0), (H.MISS_INF, 0.0), (H.MISS_NAN | H.MISS_INF | H.MISS_ABS_GE, 4.0)):
        miss = M.is_missing(x, flags, 0.0, limit)
        mask, count, filled = ctx.mask_build_nd(xd, flags, limit=limit)
        assert count == int(miss.sum()) > 0 and np.array_equal(_words(mask), N.mask_words(miss)), flags
        assert np.array_equal(_bits(filled.cpu().numpy()), _bits(N.fill(x, miss))), flags
    # under MISS_INF the signalling NaN is valid data and a source: the element behind it is not an infinity, so make it one
    y = x.copy().reshape(-1)
    y[10] = np.inf
    y = y.reshape(shape)
    miss = M.is_missing(y, H.MISS_INF)
    _, _, filled = ctx.mask_build_nd(_dev(ctx, y), H.MISS_INF)
    want = N.fill(y, miss)
    assert np.array_equal(_bits(filled.cpu().numpy()), _bits(want)) and (_bits(want) == _bits(snan)[0]).sum() >= 1


def test_refusals_leave_the_context_usable(ctx):
    """Each refusal of the contract is DCTZHIP_E_ARG before any launch: the sentinels in every buffer stay."""
    import torch
    shape = (40, 100)
    n = 4000
    x = N.field(shape, np.float64)
    xd = _dev(ctx, x)
    fbuf, fmid = _guarded(ctx, np.float64, shape)
    mbuf, mmid = _guarded_mask(ctx, n)
    count = C.c_uint64(77)
    lib, good = ctx.lib, H.Missing(H.MISS_NAN, 0.0, 0.0)
    arr = lambda *v: (C.c_size_t * len(v))(*v)

    def call(h=ctx.h, d_in=xd.data_ptr(), nd=2, dims=arr(*shape), dt=H.F64, miss=good, mask=mmid.data_ptr(), filled=fmid.data_ptr(), cnt=count):
        return lib.dctzhip_mask_build_nd(h, d_in, nd, dims, dt, C.byref(miss) if miss is not None else None, mask, filled,
                                         C.byref(cnt) if cnt is not None else None)

    for kw in (dict(h=None), dict(d_in=None), dict(miss=None), dict(mask=None), dict(cnt=None), dict(dt=2), dict(dt=-1),
               # the shape rules of compress_nd
               dict(nd=1, dims=arr(n)), dict(nd=4, dims=arr(2, 4, 5, 100)), dict(dims=None), dict(dims=arr(0, 100)), dict(dims=arr(40, 0)),
               dict(dims=arr(2 ** 31, 2)), dict(dims=arr(2 ** 16, 2 ** 16)), dict(nd=3, dims=arr(2 ** 11, 2 ** 11, 2 ** 10)),
               dict(miss=H.Missing(0, 0.0, 0.0)), dict(miss=H.Missing(16, 0.0, 0.0)), dict(miss=H.Missing(H.MISS_NAN | 32, 0.0, 0.0)),
               dict(miss=H.Missing(H.MISS_VALUE, float("nan"), 0.0)),
               dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, 0.0)), dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, -1.0)),
               dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, float("inf"))), dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, float("nan"))),
               dict(d_in=xd.data_ptr() + 8), dict(filled=fmid.data_ptr() + 8), dict(mask=mmid.data_ptr() + 4),
               dict(filled=xd.data_ptr() + 16),                                    # a partial overlap of the filled copy and the input
               dict(filled=xd.data_ptr() + 8 * (n - 2)),                           # ... by its last two elements alone
               dict(mask=xd.data_ptr() + 64), dict(mask=fmid.data_ptr() + 64)):   # the mask inside an array
        assert call(**kw) == H.E_ARG, kw
        if "h" not in kw:
            assert ctx.lib.dctzhip_last_error(ctx.h)
    assert count.value == 77
    assert _bands_untouched(fbuf, np.float64) and _mask_bands_untouched(mbuf)
    s = _bits(np.array([_sent(np.float64)]))[0]
    assert (_bits(fmid.cpu().numpy()) == s).all() and (_words(mmid) == MSENT).all()
    # a NaN value or a bad limit is only looked at when its test is selected
    assert call(miss=H.Missing(H.MISS_NAN, float("nan"), -1.0)) == H.OK and count.value == 0
    # compress_masked_nd: its own refusals, and the filled copy may not be the input
    out = ctx.alloc_outputs(ctx.nd_blocks(shape) * 64, torch.float64)
    info = H.CompressInfo()

    def cm(d_in=xd.data_ptr(), nd=2, dims=arr(*shape), eb=EB, mode=H.EC, miss=good, b=out["bin_index"].data_ptr(), mask=mmid.data_ptr(),
           filled=fmid.data_ptr(), cnt=count):
        return lib.dctzhip_compress_masked_nd(ctx.h, d_in, nd, dims, H.F64, eb, mode, C.byref(miss) if miss is not None else None, b,
                                              out["dc"].data_ptr(), out["ac_exact"].data_ptr(), mask, filled, C.byref(info),
                                              C.byref(cnt) if cnt is not None else None)

    fmid.fill_(float(_sent(np.float64)))
    mmid.fill_(MSENT)
    for kw in (dict(d_in=None), dict(miss=None), dict(b=None), dict(mask=None), dict(cnt=None), dict(mode=2), dict(nd=1), dict(dims=arr(40, 0)),
               dict(miss=H.Missing(0, 0.0, 0.0)), dict(filled=xd.data_ptr()), dict(filled=xd.data_ptr() + 16),
               dict(mask=out["bin_index"].data_ptr()), dict(filled=out["ac_exact"].data_ptr()), dict(b=out["bin_index"].data_ptr() + 8),
               dict(mask=mmid.data_ptr() + 4), dict(filled=fmid.data_ptr() + 8)):
        assert cm(**kw) == H.E_ARG, kw
    assert cm(eb=1e-7) == H.E_BOUND
    assert (_bits(fmid.cpu().numpy()) == s).all() and (_words(mmid) == MSENT).all()
    assert cm() == H.OK and info.sf == 1.0 and count.value == 0


# ---- compress_masked_nd ----------------------------------------------------------------------------------------------------
def _holey(shape, dtype):
    """Finite data with 1e36 in blobs."""
    x = N.field(shape, dtype)
    miss = N.blobs(shape)
    assert 0.2 < miss.mean() < 0.5
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


# an aligned and a ragged shape per geometry (the aligned ones are read in place by the compress kernels, the ragged ones gathered)
CM_SHAPES = ((128, 192), (125, 187), (16, 32, 48), (13, 30, 45))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("shape", CM_SHAPES, ids=["x".join(map(str, s)) for s in CM_SHAPES])
def test_compress_masked_nd_is_compress_nd_of_the_filled_array(ctx, dtype, mode, shape):
    x, miss = _holey(shape, dtype)
    n = x.size
    want_f = N.fill(x, miss)
    xd = _dev(ctx, x)
    fbuf, fmid = _guarded(ctx, dtype, shape)
    mbuf, mmid = _guarded_mask(ctx, n)
    out, info, mask, count = ctx.compress_masked_nd(xd, EB, H.MISS_VALUE, value=1e36, mode=mode, filled=fmid, mask=mmid)
    assert count == int(miss.sum()) and np.array_equal(_words(mask), N.mask_words(miss))
    assert np.array_equal(_bits(fmid.cpu().numpy()), _bits(want_f))
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), "d_in is not modified"
    assert _bands_untouched(fbuf, dtype) and _mask_bands_untouched(mbuf)
    ref_out, ref_info = ctx.compress_nd(_dev(ctx, want_f), EB, mode)
    _same_streams(out, info, ref_out, ref_info, "against ctx.compress_nd")
    # the filled copy kept by the context
    out2, info2, mask2, count2 = ctx.compress_masked_nd(xd, EB, H.MISS_VALUE, value=1e36, mode=mode)
    assert count2 == count and np.array_equal(_words(mask2), _words(mask))
    _same_streams(out2, info2, ref_out, ref_info, "context scratch")
    c = O.compress_nd(want_f, EB, mode, O.FAST)
    assert info.sf == c.sf and info.cnt == c.cnt
    assert np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)


# ---- what the layer is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(96, 160), (24, 40, 56)], ids=["2-D", "3-D"])
def test_a_tiled_field_with_1e36_holes_keeps_the_scaling_factor_of_its_valid_data(ctx, shape):
    x, miss = _holey(shape, np.float32)
    xd = _dev(ctx, x)
    _, plain = ctx.compress_nd(xd, EB, H.EC)
    assert plain.sf == float(np.float32(1e35))                           # (1e35 in the data's type)
    out, info, mask, count = ctx.compress_masked_nd(xd, EB, H.MISS_VALUE, value=1e36)
    assert count == int(miss.sum()) and info.sf == O.stats(x[~miss]).sf == 1.0
    assert info.max_abs == float(np.abs(x[~miss]).max())
    dec = ctx.decompress_nd(out, info.cnt, shape, _tdt(np.float32), EB, info.sf, H.EC)
    ctx.mask_apply(mask, x.size, FILL, dec, dims=shape, lo=[0] * len(shape), hi=shape)
    got = dec.cpu().numpy()
    assert (_bits(got[miss]) == _bits(np.array([FILL], np.float32))[0]).all()
    # every coefficient of a tile lies within eb sf of its original, so the tile's error has an L2 norm of at most sqrt(64) eb sf
    # and no element can be further off than that (plus fp32 rounding of values below 8)
    assert np.abs(got[~miss].astype(np.float64) - x[~miss]).max() <= 8 * EB * info.sf + 1e-5


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape,at", [((40, 56), (19, 30)), ((12, 16, 20), (5, 9, 14))], ids=["2-D", "3-D"])
def test_a_nan_costs_one_element_not_its_tile(ctx, dtype, shape, at):
    x = N.field(shape, dtype)
    x[at] = np.nan
    e = O.GEOM_EDGE[len(shape)]
    tile = tuple(slice(c // e * e, c // e * e + e) for c in at)
    xd = _dev(ctx, x)
    tdt = _tdt(dtype)
    out0, info0 = ctx.compress_nd(xd, EB, H.EC)
    plain = ctx.decompress_nd(out0, info0.cnt, shape, tdt, EB, info0.sf, H.EC).cpu().numpy()
    want_lost = np.zeros(shape, bool)
    want_lost[tile] = True
    assert np.array_equal(np.isnan(plain), want_lost) and want_lost.sum() == 64
    out, info, mask, count = ctx.compress_masked_nd(xd, EB, H.MISS_NAN)
    assert count == 1
    dec = ctx.decompress_nd(out, info.cnt, shape, tdt, EB, info.sf, H.EC)
    assert not np.isnan(dec.cpu().numpy()).any()
    ctx.mask_apply(mask, x.size, float("nan"), dec, dims=shape, lo=[0] * len(shape), hi=shape)
    got = dec.cpu().numpy()
    lost = np.isnan(got)
    assert lost.sum() == 1 and lost[at]
    ok = ~np.isnan(x)
    assert np.abs(got[ok].astype(np.float64) - x[ok]).max() <= 8 * EB * info.sf + 1e-5      # (sqrt(64) eb sf, as above)


CG = {(61, 93): ((3, 10), (58, 77)), (13, 30, 45): ((1, 2, 3), (11, 27, 42))}          # shape -> a box that cuts tiles on every side


@pytest.mark.parametrize("dtype,mode", [(np.float64, H.EC), (np.float32, H.QT)], ids=["float64-EC", "float32-QT"])
@pytest.mark.parametrize("shape", list(CG), ids=["2-D", "3-D"])
def test_composed_guarantee(ctx, dtype, mode, shape):
    """compress_masked_nd, the correction list against the FILLED array, decompress_nd or a decompress_box_nd box that cuts tiles,
    fixup_apply_nd, then mask_apply: every valid element has the original's bits or lies within the bound (compared in T), every
    missing element the fill's bits, and nothing outside the box is written."""
    x, miss = _holey(shape, dtype)
    miss |= N.pattern("random30", shape)
    x[miss] = 1e36
    n, tdt = x.size, _tdt(dtype)
    xd = _dev(ctx, x)
    filled = ctx.torch.empty_like(xd)
    out, info, mask, count = ctx.compress_masked_nd(xd, EB, H.MISS_VALUE, value=1e36, mode=mode, filled=filled)
    assert count == int(miss.sum())
    q = np.array(info.qtable[:]) if mode == H.QT else None
    sf, cnt = info.sf, info.cnt
    idx, tot = ctx.ac_index(out, ctx.nd_blocks(shape) * 64)
    assert tot == cnt
    bound = 0.1 * EB * sf                     # (well inside the quantisation error of either geometry: the list is not empty)
    fix = ctx.fixup_build_nd(out, cnt, shape, tdt, EB, sf, filled, bound, index=idx, mode=mode, qtable=q)
    assert fix[3] > 0
    fillbits = _bits(np.array([FILL], dtype))[0]

    def check(got, sl, what):
        xs, ms = x[sl].reshape(-1), miss[sl].reshape(-1)
        got = got.reshape(-1)
        same = _bits(got) == _bits(xs)
        with np.errstate(invalid="ignore", over="ignore"):
            near = np.abs(xs - got) <= dtype(bound)
        assert bool((same | near)[~ms].all()), what
        assert bool((_bits(got)[ms] == fillbits).all()), what
        assert ms.any() and (~ms).any(), what

    whole = ctx.decompress_nd(out, cnt, shape, tdt, EB, sf, mode, qtable=q)
    ctx.fixup_apply_nd(fix, shape, tdt, whole)
    ctx.mask_apply(mask, n, FILL, whole, dims=shape, lo=[0] * len(shape), hi=shape)
    check(whole.cpu().numpy(), tuple(slice(None) for _ in shape), "whole")
    lo, hi = CG[shape]
    ext = tuple(h - l for l, h in zip(lo, hi))
    buf, mid = _guarded(ctx, dtype, ext)
    ctx.decompress_box_nd(out, cnt, shape, tdt, EB, sf, lo, hi, idx, mode=mode, qtable=q, dst=mid)
    ctx.fixup_apply_nd(fix, shape, tdt, mid, lo=lo, hi=hi)
    ctx.mask_apply(mask, n, FILL, mid, dims=shape, lo=lo, hi=hi)
    check(mid.cpu().numpy(), tuple(slice(l, h) for l, h in zip(lo, hi)), "box")
    assert _bands_untouched(buf, dtype)
