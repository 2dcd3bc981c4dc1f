"""NaN and Inf inputs on every compress and decode path, against the oracle under the device ABI's rule
(tests/nonfinite.py has the kinds and the comparison rule).

  * a NaN coefficient gets bin id 0 -- not in AC_exact, not in the QT table -- and its block decodes to NaN;
  * the statistics pass a NaN over wherever it stands (x[0] included): one NaN costs one block, never the array;
  * an infinity gives sf = inf, cnt = 0 and an all-NaN decode, as util.c:29 has it;
  * integer streams and header scalars are exact, floating-point streams are NaN exactly where the oracle's are
    (sign and payload free) and bit-identical everywhere else.
Every case is one call with a normal exit."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import nonfinite as NF
from tests import workloads as W
from tests.test_gpu_parity import _sampled_chunk, _unsampled_element
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

EB = 1e-3
N_BIG = (1 << 22) + 64 * 11 + 5            # several tiles per workgroup of the persistent kernels, a short last block
N_ONE = 64 * 64 * 3 + 64 * 9 + 21          # a few tiles: one launch by default
N_TINY = 40                                # shorter than a block
N_SPEC = 1 << 20
DTYPES = [np.float64, np.float32]
MODES = [O.EC, O.QT]
_MODE_ID = {O.EC: "EC", O.QT: "QT"}


def _ids(v):
    if isinstance(v, type) and issubclass(v, np.floating):
        return np.dtype(v).name
    return None


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain():
    import dctz_amd
    c = dctz_amd.Context(0)
    c.set_one_launch(False)
    yield c
    c.close()


@pytest.fixture()
def spec_ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    c.set_speculation(True, 1 << 18)
    c.set_one_launch(False)
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


@functools.lru_cache(maxsize=64)
def _oracle(kind, n, dtname, mode):
    """(x, poisoned blocks, the oracle's streams under the device ABI's rule, its decode) -- and, for the kinds whose
    damage is contained, the budget of NaNs asserted from the oracle alone."""
    x, bad = NF.make(kind, n, np.dtype(dtname).type)
    c = O.compress(x, EB, mode, O.FAST, nan_rule=O.NAN_SKIP)
    r = O.decompress(c, O.FAST)
    if kind in NF.CONTAINED:
        NF.contained_budget(c, r, bad.size)
    if kind == "snan_after_max":
        assert c.sf == 1000.0 and c.stats.max == NF.SPIKE
    if kind in NF.INF_KINDS:
        assert c.sf == np.inf and c.cnt == 0 and np.isnan(r).all()
    x.setflags(write=False)
    return x, bad, c, r


def _eq(got, want, what):
    assert NF.same_with_nans(got, want), f"{what}: {NF.describe_mismatch(got, want)}"


def _scalar_same(a, b):
    return a == b or (a != a and b != b)


def _check_mean(info_mean, c):
    if np.isfinite(c.mean):
        assert np.isfinite(info_mean) and abs(info_mean - c.mean) <= 1e-5 * max(1.0, abs(c.mean)), (info_mean, c.mean)
    else:
        assert not np.isfinite(info_mean), (info_mean, c.mean)


def _check_streams(out, info, c, mode, dtype, stats=True):
    """The comparison rule: bin_index, cnt, sf, max|x|, min|x| exact; DC, AC_exact[:cnt], the QT table NaN where the oracle's."""
    assert info.sf == c.sf, (info.sf, c.sf)
    if stats:
        assert info.max_abs == c.stats.max and info.min_abs == c.stats.min, (info.max_abs, c.stats.max, info.min_abs, c.stats.min)
        _check_mean(info.mean, c)
    assert info.cnt == c.cnt, (info.cnt, c.cnt)
    got = out["bin_index"].cpu().numpy()
    bad = np.flatnonzero(got != c.bin_index)
    assert bad.size == 0, f"bin_index: {bad.size} mismatches, first at {bad[:6]}: got {got[bad[:6]]} want {c.bin_index[bad[:6]]}"
    _eq(out["dc"].cpu().numpy(), c.dc, "dc")
    _eq(out["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact, "ac_exact")
    if mode == O.QT:
        _eq(np.array(info.qtable[:], dtype=dtype), c.qtable, "qtable")
        _eq(np.array(info.qtable_raw[:], dtype=dtype), c.qtable_raw, "qtable_raw")


def _decode(ctx, out, info, n, dtype, mode):
    return ctx.decompress(out, info.cnt, n, _tdt(dtype), EB, info.sf, mode, qtable=np.array(info.qtable[:])).cpu().numpy()


def _roundtrip(ctx, kind, n, dtype, mode, want_flag=None, **kw):
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, mode)
    xd = _dev(ctx, x)
    out, info = ctx.compress(xd, EB, mode, **kw)
    if want_flag is not None:
        assert info.flags & want_flag, hex(info.flags)
    _check_streams(out, info, c, mode, dtype)
    _eq(_decode(ctx, out, info, n, dtype, mode), ref, "decode")
    return x, xd, out, info, c, ref


# ---- the large-array path: persistent k_compress / k_decompress(_il), statistics behind a sampled guess -----------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("kind", NF.KINDS)
def test_large_array_path(chain, kind, mode, dtype):
    """(An MI355X holds all the tiles of an array of this size at once, so by default it is a one-launch call: the persistent
    kernels take it on a context with one-launch off, statistics behind the sampled guess as by default.)"""
    x, xd, out, info, c, ref = _roundtrip(chain, kind, N_BIG, dtype, mode)
    assert not (info.flags & H.INFO_ONE_LAUNCH)
    names = (chain.last_kernel(0), chain.last_kernel(1))
    assert names[0].startswith("k_compress") and names[1].startswith("k_decompress") and not any("_one" in k for k in names), names
    assert NF.same_with_nans(xd.cpu().numpy(), x), "input must not be modified"


# ---- the one-launch kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [(N_ONE, np.float64), (N_ONE, np.float32), (N_TINY, np.float64), (N_TINY, np.float32), (N_BIG, np.float32)],
                         ids=lambda v: _ids(v) or str(v))
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("kind", NF.KINDS)
def test_one_launch_kernels(ctx, kind, n, mode, dtype):
    """k_compress_one / k_decompress_one took the call (a call the kernel hands back to the chain would pass on the chain's
    merits), and the context still takes the next one.  (N_BIG: 16 MiB of fp32 are still all resident at once on an MI355X,
    32 MiB of fp64 are not.)"""
    _roundtrip(ctx, kind, n, dtype, mode, want_flag=H.INFO_ONE_LAUNCH)
    assert ctx.last_kernel(1).startswith("k_decompress_one")
    y = W.ragged(n, dtype, scale=37.0)
    out, info = ctx.compress(_dev(ctx, y), EB, mode)
    assert info.flags & H.INFO_ONE_LAUNCH, "a non-finite input must not switch the one-launch path off for the context"
    k = O.compress(y, EB, mode, O.FAST)
    _check_streams(out, info, k, mode, dtype)


# ---- the chain of kernels on the same sizes: k_compress, and the two-wavefront kernel with and without single-pass placement
@pytest.mark.parametrize("dtype,split", [(np.float64, 0), (np.float32, 0), (np.float64, 1), (np.float64, 3)],
                         ids=["float64-split0", "float32-split0", "float64-split1", "float64-split3"])
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("n", [N_ONE, N_TINY])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_chain_and_two_wavefront_kernel(chain, kind, n, mode, dtype, split):
    chain.set_split(split)
    try:
        x, xd, out, info, c, ref = _roundtrip(chain, kind, n, dtype, mode)
    finally:
        chain.set_split(False)
    assert not (info.flags & H.INFO_ONE_LAUNCH)
    if n >= 64:
        assert bool(info.flags & H.INFO_SPLIT) == (split != 0), hex(info.flags)
    if split == 3 and mode == O.EC and n >= 4096:
        assert info.flags & H.INFO_SINGLE_PASS


# ---- speculation: the sampled guess of the decade and its verification ---------------------------------------------------
def _spec_position(dtype, sampled, group_index=5):
    chunk_elems = 256 * (16 // np.dtype(dtype).itemsize)
    if sampled:
        return _sampled_chunk(group_index) * chunk_elems + 17
    return _unsampled_element(dtype, group_index)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("sampled", [True, False], ids=["sampled", "unsampled"])
@pytest.mark.parametrize("what", ["qnan", "snan_behind_spike", "pos_inf", "neg_inf"])
def test_speculation(spec_ctx, what, sampled, mode, dtype):
    """A NaN / an infinity where the sample reads and where it does not.  Either the guess verifies or the miss is detected
    and the call runs again: the flags say which, and sf is the oracle's either way -- never a silently wrong one."""
    x = W.ragged(N_SPEC, dtype, scale=37.0)
    p = _spec_position(dtype, sampled)
    dt = np.dtype(dtype)
    if what == "qnan":
        NF.put_bits(x, p, NF._QNAN[dt])
    elif what == "snan_behind_spike":                 # the array's maximum, then signalling NaNs in the same 16-byte vector / block
        p -= p % 4
        x[p] = NF.SPIKE
        NF.put_bits(x, np.array([p + 1, p + 2, p + 3, p + 9]), NF._SNAN[dt])
    else:
        x[p] = np.inf if what == "pos_inf" else -np.inf
    c = O.compress(x, EB, mode, O.FAST, nan_rule=O.NAN_SKIP)
    ref = O.decompress(c, O.FAST)
    assert c.sf == {"qnan": 10.0, "snan_behind_spike": 1000.0}.get(what, np.inf)
    out, info = spec_ctx.compress(_dev(spec_ctx, x), EB, mode)
    assert info.flags in (H.INFO_STATS_FUSED, H.INFO_RESPUN), hex(info.flags)
    if what == "qnan":
        assert info.flags == H.INFO_STATS_FUSED, "a NaN is passed over: the guess stands"
    if not sampled and what != "qnan":
        assert info.flags == H.INFO_RESPUN, "the sample cannot have seen it"
    _check_streams(out, info, c, mode, dtype)
    _eq(_decode(spec_ctx, out, info, N_SPEC, dtype, mode), ref, "decode")


# ---- the scaled copy, in a buffer of its own and over the input ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("in_place", [False, True], ids=["scaled_copy", "in_place"])
@pytest.mark.parametrize("n", [N_ONE, (1 << 20) + 64 * 3 + 9])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_scaled_copy_and_in_place_scaling(ctx, kind, n, in_place, mode, dtype):
    import torch
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, mode)
    xd = _dev(ctx, x)
    scaled = xd if in_place else torch.empty_like(xd)
    out, info = ctx.compress(xd, EB, mode, scaled=scaled)
    _check_streams(out, info, c, mode, dtype)
    _eq(scaled.cpu().numpy(), c.scaled, "x / sf")
    if not in_place:
        assert NF.same_with_nans(xd.cpu().numpy(), x), "input must not be modified"


# ---- compress_part with the whole array's statistics ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", NF.KINDS)
def test_parts_with_the_arrays_statistics(ctx, kind, dtype):
    n, part = N_ONE, 64 * 64 + 64 * 3
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, O.EC)
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    for k in out:
        out[k].zero_()
    S, lo = 0, 0
    while lo < n:
        ne = min(part, n - lo)
        px = O.stats(x[lo:lo + ne], O.NAN_SKIP)
        cnt, st, sf = ctx.compress_part(xd[lo:lo + ne], EB, c.stats.max, c.stats.min, out, lo, S)
        assert sf == c.sf and st[0] == px.max and st[1] == px.min, (lo, sf, st, px.max, px.min)
        S += cnt
        lo += ne
    whole, winfo = ctx.compress(xd, EB, O.EC)
    assert S == c.cnt == winfo.cnt
    assert np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)
    _eq(out["dc"].cpu().numpy(), c.dc, "dc")
    _eq(out["ac_exact"][:S].cpu().numpy(), c.ac_exact, "ac_exact")
    assert np.array_equal(out["bin_index"].cpu().numpy(), whole["bin_index"].cpu().numpy()), "the parts equal the one call"
    _eq(out["ac_exact"][:S].cpu().numpy(), whole["ac_exact"][:S].cpu().numpy(), "ac_exact against the one call")


# ---- batches ------------------------------------------------------------------------------------------------------------
def _solo(ctx, xd, eb, mode):
    out, info = ctx.compress(xd, eb, mode)
    return {k: v.clone() for k, v in out.items()}, (info.sf, info.cnt, info.max_abs, info.min_abs, list(info.qtable[:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("one", [True, False], ids=["one_launch", "chain"])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_batch_with_a_poisoned_item_between_clean_ones(ctx, kind, one, mode, dtype):
    """[clean, poisoned, clean, poisoned under a second bound (the same input: one statistics pass serves both bounds)]:
    the clean items are bit-identical to their solo results, the poisoned ones the oracle's; then the decode side."""
    import torch
    n = 64 * 90 + 33
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, mode)
    c2 = O.compress(x, 1e-4, mode, O.FAST, nan_rule=O.NAN_SKIP)
    a, b = W.ragged(64 * 70 + 5, dtype, scale=37.0), W.ragged(64 * 120 + 63, dtype, seed=3, scale=5.0)
    ad, bd, xd = _dev(ctx, a), _dev(ctx, b), _dev(ctx, x)
    ctx.set_one_launch(one)
    try:
        sa, ia = _solo(ctx, ad, EB, mode)
        sb, ib = _solo(ctx, bd, EB, mode)
        outs, infos, _ = ctx.compress_batch([ad, xd, bd, xd], [EB, EB, EB, 1e-4], mode)
        torch.cuda.synchronize()
        for o, i, (so, si) in ((outs[0], infos[0], (sa, ia)), (outs[2], infos[2], (sb, ib))):
            assert (i.sf, i.cnt, i.max_abs, i.min_abs, list(i.qtable[:])) == si
            assert torch.equal(o["bin_index"], so["bin_index"]) and torch.equal(o["dc"].view(torch.int32), so["dc"].view(torch.int32))
            assert torch.equal(o["ac_exact"][:i.cnt].view(torch.int32), so["ac_exact"][:i.cnt].view(torch.int32))
        _check_streams(outs[1], infos[1], c, mode, dtype)
        _check_streams(outs[3], infos[3], c2, mode, dtype)
        ns, ebs = [a.size, n, b.size, n], [EB, EB, EB, 1e-4]
        recs, status, _ = ctx.decompress_batch(outs, [i.cnt for i in infos], ns, [_tdt(dtype)] * 4, ebs, [i.sf for i in infos], mode,
                                               qtables=[np.array(i.qtable[:]) for i in infos])
        assert list(status) == [0] * 4
        for j, (src, i) in enumerate(((a, infos[0]), (b, infos[2]))):
            k = O.compress(src, EB, mode, O.FAST)
            assert np.array_equal(recs[2 * j].cpu().numpy().view(np.uint8), O.decompress(k, O.FAST).view(np.uint8))
        _eq(recs[1].cpu().numpy(), ref, "decode of the poisoned item")
        _eq(recs[3].cpu().numpy(), O.decompress(c2, O.FAST), "decode of the poisoned item at the second bound")
    finally:
        ctx.set_one_launch(True)


# ---- multi-dimensional blocks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("shape", [(8 * 21 + 3, 8 * 19 + 5), (4 * 9 + 1, 4 * 11 + 2, 4 * 13)], ids=["8x8", "4x4x4"])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_multi_dimensional_blocks(ctx, kind, shape, mode, dtype):
    n = int(np.prod(shape))
    x = NF.make(kind, n, dtype)[0].reshape(shape)
    c = O.compress_nd(x, EB, mode, O.FAST, nan_rule=O.NAN_SKIP)
    ref = O.decompress_nd(c, shape, O.FAST)
    if kind in NF.CONTAINED:
        nbad = np.unique(np.flatnonzero(~np.isfinite(O.nd_gather(x))) // 64).size
        NF.contained_budget(c, O.decompress(c, O.geom_impl(len(shape), O.FAST)), nbad)
    out, info = ctx.compress_nd(_dev(ctx, x), EB, mode)
    _check_streams(out, info, c, mode, dtype)
    r = ctx.decompress_nd(out, info.cnt, shape, _tdt(dtype), EB, info.sf, mode, qtable=np.array(info.qtable[:])).cpu().numpy()
    _eq(r, ref, "decode")


# ---- random access ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES, ids=_MODE_ID.get)
@pytest.mark.parametrize("kind", NF.KINDS)
def test_random_access_around_a_poisoned_tile(ctx, kind, mode, dtype):
    """ac_index / decompress_range over ranges that start before, inside and behind the poisoned tile: each the slice of
    the whole decode (itself the oracle's) under the same NaN rule."""
    n = 4096 * 6 + 64 * 3 + 17
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, mode)
    out, info = ctx.compress(_dev(ctx, x), EB, mode)
    _check_streams(out, info, c, mode, dtype)
    idx, tot = ctx.ac_index(out, n)
    assert tot == c.cnt
    flags = (c.bin_index == 255) & (np.arange(n) % 64 != 0)
    cs = np.concatenate([[0], np.cumsum(flags, dtype=np.int64)])
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), cs[np.minimum(np.arange(-(-n // 4096) + 1) * 4096, n)])
    t = int(bad[len(bad) // 2]) // 64                       # a poisoned tile
    lo_t, hi_t = 4096 * t, min(4096 * t + 4096, n)
    ranges = [(0, n), (max(lo_t - 100, 0), lo_t + 7), (max(lo_t - 4096, 0), hi_t), (lo_t, hi_t), (lo_t + 70, min(lo_t + 200, n)),
              (lo_t + 64 * 17 + 3, min(hi_t + 130, n)), (min(hi_t, n - 1), n), (min(hi_t + 64, n - 1), min(hi_t + 64 + 500, n)), (n - 5, n)]
    q = np.array(info.qtable[:])
    for lo, hi in ranges:
        if not (0 <= lo < hi <= n):
            continue
        r = ctx.decompress_range(out, info.cnt, n, _tdt(dtype), EB, info.sf, lo, hi, idx, mode, qtable=q).cpu().numpy()
        assert NF.same_with_nans(r, ref[lo:hi]), f"range [{lo}, {hi}): {NF.describe_mismatch(r, ref[lo:hi])}"


# ---- the block transform on its own -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_block_transform(ctx, kind, inverse, dtype):
    """dct_blocks on blocks holding NaN, +Inf, -Inf: the NaN mask of the oracle's pinned flow (an infinity leaves infinities
    and NaNs behind, by the same expression tree), finite blocks bit-exact."""
    n = 64 * 37 + 40
    x, bad = NF.make(kind, n, dtype)
    y = ctx.dct_blocks(_dev(ctx, x), inverse=inverse).cpu().numpy()
    ref = np.empty_like(x)
    for b in range((n + 63) // 64):
        sl = slice(64 * b, min(n, 64 * b + 64))
        with np.errstate(all="ignore"):
            ref[sl] = O.dct_inv(x[sl], O.FAST) if inverse else O.dct_fwd(x[sl], O.FAST)
    keep = np.ones(n, bool)
    for b in bad:
        keep[64 * b:64 * b + 64] = False
    assert not np.isnan(ref[keep]).any() and np.array_equal(y[keep].view(np.uint8), ref[keep].view(np.uint8)), "finite blocks bit-exact"
    _eq(y, ref, "transform")


# ---- the statistics on their own ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n", [N_ONE, N_TINY, (1 << 20) + 64 * 3 + 9])
@pytest.mark.parametrize("kind", NF.KINDS)
def test_statistics_agree(ctx, chain, kind, n, dtype):
    """dctzhip_stats, the statistics compress reports (one launch / chain / behind a sampled guess) and the oracle's."""
    x, bad, c, ref = _oracle(kind, n, np.dtype(dtype).name, O.EC)
    xd = _dev(ctx, x)
    st = H.CompressInfo()
    ctx._bind_stream()
    assert ctx.lib.dctzhip_stats(ctx.h, xd.data_ptr(), n, H.F64 if dtype == np.float64 else H.F32, C.byref(st)) == 0
    want = (c.stats.max, c.stats.min, c.sf)
    assert (st.max_abs, st.min_abs, st.sf) == want, ((st.max_abs, st.min_abs, st.sf), want)
    _check_mean(st.mean, c)
    for cx in (ctx, chain):
        _, info = cx.compress(_dev(cx, x), EB, O.EC)
        assert (info.max_abs, info.min_abs, info.sf) == want, ((info.max_abs, info.min_abs, info.sf), want)
        _check_mean(info.mean, c)


# ---- callers that must refuse or report ----------------------------------------------------------------------------------------
RD_EBS = [1e-2, 1e-3, 1e-4, 1e-5]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n", [N_ONE, (1 << 20) + 64 * 3 + 9])
def test_rd_probe_counts_with_a_nan(ctx, n, dtype):
    x, bad = NF.make("qnan_one", n, dtype)
    d = _dev(ctx, x)
    pts, rng = ctx.rd_probe(d, RD_EBS)
    for eb, p in zip(RD_EBS, pts):
        _, info = ctx.compress(d, eb, O.EC)
        want = O.compress(x, eb, O.EC, O.FAST, nan_rule=O.NAN_SKIP).cnt
        assert p["cnt"] == info.cnt == want, (eb, p["cnt"], info.cnt, want)
        assert p["raw_bytes"] == n + 4 * ((n + 63) // 64) + 4 * info.cnt + 56
        assert np.isnan(p["sse"]), "the distortion of an array with a NaN is a NaN, not a number"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", NF.KINDS)
def test_compress_psnr_refuses_and_the_context_goes_on(ctx, kind, dtype):
    import torch
    n = 64 * 500 + 7
    x, bad = NF.make(kind, n, dtype)
    d = _dev(ctx, x)
    out = ctx.alloc_outputs(n)
    for v in out.values():
        v.view(torch.uint8).fill_(0xA5)
    info, eb, ps = H.CompressInfo(), C.c_double(-7.0), C.c_double(-7.0)
    ctx._bind_stream()
    rc = ctx.lib.dctzhip_compress_psnr(ctx.h, d.data_ptr(), n, H.F64 if dtype == np.float64 else H.F32, 40.0,
                                       out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                       C.byref(info), C.byref(eb), C.byref(ps))
    torch.cuda.synchronize()
    assert rc == H.E_ARG, rc
    assert all(bool((v.view(torch.uint8) == 0xA5).all()) for v in out.values()) and eb.value == -7.0 and ps.value == -7.0
    y = W.ragged(n, dtype, scale=37.0)                     # the next call on the same context, clean data
    k = O.compress(y, EB, O.EC, O.FAST)
    o2, i2 = ctx.compress(_dev(ctx, y), EB, O.EC)
    _check_streams(o2, i2, k, O.EC, dtype)
    assert np.array_equal(_decode(ctx, o2, i2, n, dtype, O.EC).view(np.uint8), O.decompress(k, O.FAST).view(np.uint8))
    _, _, eb2, ps2 = ctx.compress_psnr(_dev(ctx, y), 40.0)
    assert eb2 in H.psnr_grid() and ps2 >= 40.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_psnr_terms_on_a_reconstruction_with_a_nan_block(ctx, dtype):
    n = N_ONE
    x, bad, c, ref = _oracle("qnan_one", n, np.dtype(dtype).name, O.EC)
    clean = W.ragged(n, dtype, scale=37.0)
    t = ctx.psnr_terms(_dev(ctx, clean), _dev(ctx, ref))
    assert t[0] == float(clean.min()) and t[1] == float(clean.max())
    assert np.isnan(O.psnr(clean, ref)["rmse"]) and np.isnan(t[3]), "the sum of squared errors over a NaN block is a NaN (util.c:78-79)"
