"""The decode memo (include/dctz_hip.h: dctzhip_set_decode_memo).

A dctzhip_decompress of exactly the streams the context's last dctzhip_compress wrote starts from that call's per-tile
tables (counts of exact coefficients, their first places in AC_exact[]) instead of a counting pass over bin_index, and the
decoder checks every count against the flags it reads.  Checked here: a hit is bit for bit the oracle's and the classic
decoder's reconstruction; a memo made stale by rewriting the buffers is found, decoded again the classic way inside the same
call, and an under-run is still refused; everything the memo does not apply to, and everything that invalidates it, takes
the classic kernel.  The references are the oracle (FAST) and a second context with DCTZHIP_DEC_MEMO=0, never the memo path.

All on the chain of kernels (set_one_launch(False)), fp64, EC, eb 1e-3.  Sizes: 1, 3 and 1100 tiles of 4096 elements --
1100 gives 76 workgroups of a 1024-workgroup decode grid a second tile (a larger grid: grid + 76 tiles).  The stale-memo
case that moves a flag between two tiles needs two tiles and so runs on the sizes 3 and 1100 only; the one-tile size has
its stale memo in the under-run case."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE = 4096
EB = 1e-3
MEMO, REDO = 16, 17                     # dctzhip_debug_counter: memo decodes, stale redos
MEMO_KERNEL = "k_decompress_il<double, 0, 1, true>"


def _make(env):
    import dctz_amd
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = dctz_amd.Context(0)         # (the knobs are read when the context is created)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_one_launch(False)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _make({})
    yield c
    c.close()


@pytest.fixture(scope="module")
def classic():
    c = _make({"DCTZHIP_DEC_MEMO": "0"})
    yield c
    c.close()


def _grid():
    """Workgroups of the fp64 decode launch of a large array: four single-wave workgroups per CU (their LDS)."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _sizes():
    import torch
    big = 1100
    if torch.cuda.is_available() and _grid() > 1024:
        big = _grid() + 76
    return [1, 3, big]


SIZES = _sizes()


def field(n, dtype=np.float64, seed=11):
    """A smooth field whose amplitude drifts from tile to tile, plus noise: every tile stores some coefficients exactly
    (the low frequencies of its blocks), and not the same number everywhere.  Two tiles of three carry a block with an
    alternating burst (exact coefficients at the highest frequencies: a list k_compact_ac has to walk, where a smooth
    tile's list is copied as it stands), and tile 1 is bounded noise (more exact coefficients than the decoder stages
    ahead: 1024).  max|x| stays below 100, so the scaling factor is 100 throughout."""
    t = np.arange(n) / 61.0
    rng = np.random.default_rng(seed + n)
    amp = 30.0 + 12.0 * np.sin(np.arange(n) / 9973.0)
    v = amp * (np.sin(t) + 0.3 * np.cos(5.3 * t)) + 0.4 * rng.standard_normal(n)
    burst = 30.0 * (1.0 - 2.0 * (np.arange(64) % 2))
    for tile in range(n // TILE):
        if tile % 3 != 2:
            v[tile * TILE + 5 * 64:tile * TILE + 6 * 64] += burst
    if n >= 2 * TILE:
        v[TILE:2 * TILE] = rng.uniform(-95.0, 95.0, TILE)
    return v.astype(dtype)


def tile_counts(bin_index):
    """Per tile: flags 'stored exactly' (id 255 at j != 0) of the full blocks."""
    nfull = bin_index.size // 64
    b = bin_index[:nfull * 64].reshape(nfull, 64)
    per_block = (b[:, 1:] == 255).sum(axis=1)
    pad = (-nfull) % 64
    return np.concatenate([per_block, np.zeros(pad, per_block.dtype)]).reshape(-1, 64).sum(axis=1)


@functools.lru_cache(maxsize=None)
def case(n, dtype=np.float64, mode=O.EC):
    """Input, the oracle's streams and its reconstruction; computed once, never modified."""
    x = field(n, dtype)
    c = O.compress(x, EB, mode, O.FAST)
    ref = O.decompress(c, O.FAST)
    for a in (x, c.bin_index, c.dc, c.ac_exact, ref):
        a.setflags(write=False)
    return x, c, ref


def assert_input_exercises_the_memo(c, ntiles):
    """On the CPU, before any GPU call: the per-tile counts are non-zero and, in every round of the decode grid that has
    more than one tile, not all equal (a memo of equal counts could not tell one tile's start from another's)."""
    cnt = tile_counts(c.bin_index)
    assert cnt.size == ntiles and int(cnt.sum()) == c.cnt and (cnt > 0).all()
    g = min(_grid(), ntiles)
    for r0 in range(0, ntiles, g):
        rnd = cnt[r0:r0 + g]
        if rnd.size > 1:
            assert np.unique(rnd).size > 1, (r0, rnd[:8])


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(ctx.device)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _counters(ctx):
    return ctx.counter(MEMO), ctx.counter(REDO)


def _raw_decompress(ctx, out, cnt, n, sf, dst):
    ctx._bind_stream()
    return ctx.lib.dctzhip_decompress(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                      int(cnt), None, n, H.F64, float(EB), float(sf), H.EC, dst.data_ptr())


def _write_streams(out, bin_index, ac):
    """Rewrites the device buffers in place (same pointers) on the stream the context works on."""
    import torch
    out["bin_index"].copy_(torch.from_numpy(np.array(bin_index, copy=True)))
    if ac.size:
        out["ac_exact"][:ac.size].copy_(torch.from_numpy(np.array(ac, copy=True)))


def _modified(c, bin_index, ac):
    m = O.Compressed()
    for k in O.Compressed.__slots__:
        setattr(m, k, getattr(c, k, None) if hasattr(c, k) else None)
    m.bin_index, m.ac_exact, m.cnt = bin_index, ac, ac.size
    return m


def _flag_positions(bin_index):
    """Indices of the flagged elements, in stream order (= the order of their entries in AC_exact[])."""
    j = np.arange(bin_index.size) % 64
    return np.flatnonzero((bin_index == 255) & (j != 0))


# ---- 1. hit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", SIZES)
def test_hit_is_bit_exact_and_repeats(ctx, classic, ntiles):
    n = ntiles * TILE
    x, c, ref = case(n)
    assert_input_exercises_the_memo(c, ntiles)
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n)
    m0, r0 = _counters(ctx)
    recs = []
    for k in range(3):                                    # (three pairs: the arrival word has to be back at zero every time)
        _, info = ctx.compress(xd, EB, H.EC, out=out)
        assert not (info.flags & H.INFO_ONE_LAUNCH) and info.cnt == c.cnt and info.sf == c.sf
        rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC)
        assert ctx.last_kernel(1) == MEMO_KERNEL
        assert _counters(ctx) == (m0 + k + 1, r0)
        recs.append(rec.cpu().numpy())
    assert np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)
    assert _same(out["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact)
    cm0 = classic.counter(MEMO)
    want = classic.decompress(out, c.cnt, n, _tdt(np.float64), EB, c.sf, H.EC).cpu().numpy()
    assert classic.counter(MEMO) == cm0 and "true" not in classic.last_kernel(1)
    for rec in recs:
        assert _same(rec, ref) and _same(rec, want)


# ---- 2. stale memo, same total ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", [s for s in SIZES if s >= 2])
def test_stale_memo_with_the_same_total_is_decoded_again(ctx, classic, ntiles):
    n = ntiles * TILE
    x, c, _ = case(n)
    assert_input_exercises_the_memo(c, ntiles)
    g = min(_grid(), ntiles)
    # one flag moves from tile a (first round of the grid) to tile b (second round where there is one, else the last tile)
    a, b = 0, (g if ntiles > g else ntiles - 1)
    assert a != b
    bin2 = c.bin_index.copy()
    flags = _flag_positions(bin2)
    e1 = int(flags[(flags >= a * TILE) & (flags < (a + 1) * TILE)][0])
    k1 = int(np.searchsorted(flags, e1))                  # its entry in AC_exact[]
    bin2[e1] = 0
    ac2 = np.delete(c.ac_exact, k1)
    tb = bin2[b * TILE:(b + 1) * TILE]
    free = np.flatnonzero((tb != 255) & (np.arange(TILE) % 64 != 0))
    e2 = b * TILE + int(free[free.size // 2])
    bin2[e2] = 255
    k2 = int(np.searchsorted(_flag_positions(bin2), e2))
    ac2 = np.insert(ac2, k2, np.float32(0.125))
    assert ac2.size == c.cnt and int(tile_counts(bin2).sum()) == c.cnt
    assert tile_counts(bin2)[a] == tile_counts(c.bin_index)[a] - 1 and tile_counts(bin2)[b] == tile_counts(c.bin_index)[b] + 1
    want_orc = O.decompress(_modified(c, bin2, ac2), O.FAST)

    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n)
    _, info = ctx.compress(xd, EB, H.EC, out=out)
    assert info.cnt == c.cnt
    _write_streams(out, bin2, ac2)
    m0, r0 = _counters(ctx)
    rec = ctx.decompress(out, c.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()    # returns OK
    assert _counters(ctx) == (m0 + 1, r0 + 1)
    assert "true" not in ctx.last_kernel(1)               # the kernel that made the result is the classic one
    want = classic.decompress(out, c.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    assert _same(rec, want_orc) and _same(rec, want)
    # the next pair is a clean hit
    x0, c0, ref0 = case(n)
    _, info = ctx.compress(xd, EB, H.EC, out=out)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    assert _counters(ctx) == (m0 + 2, r0 + 1) and ctx.last_kernel(1) == MEMO_KERNEL
    assert _same(rec, ref0)


# ---- 3. stale memo that under-runs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", SIZES)
def test_stale_memo_that_under_runs_is_refused(ctx, ntiles):
    import torch
    n = ntiles * TILE
    x, c, ref = case(n)
    assert_input_exercises_the_memo(c, ntiles)
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n)
    _, info = ctx.compress(xd, EB, H.EC, out=out)
    bin2 = c.bin_index.copy()
    t = ntiles - 1                                        # flags added to the last tile, no coefficients added
    tb = bin2[t * TILE:(t + 1) * TILE]
    free = np.flatnonzero((tb != 255) & (np.arange(TILE) % 64 != 0))[:5]
    tb[free] = 255
    _write_streams(out, bin2, np.empty(0, np.float32))
    dst = torch.empty(n, dtype=torch.float64, device=ctx.device)
    m0, r0 = _counters(ctx)
    assert _raw_decompress(ctx, out, c.cnt, n, info.sf, dst) == H.E_ARG
    assert _counters(ctx) == (m0 + 1, r0 + 1)
    # the next good call succeeds: the intact streams again, first classic (no memo stands), then a pair that hits
    _write_streams(out, c.bin_index, np.empty(0, np.float32))
    rec = ctx.decompress(out, c.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    assert _counters(ctx) == (m0 + 1, r0 + 1) and _same(rec, ref)
    _, info = ctx.compress(xd, EB, H.EC, out=out)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    assert _counters(ctx) == (m0 + 2, r0 + 1) and _same(rec, ref)


# ---- 4. does not apply --------------------------------------------------------------------------------------------------
def _expect_classic(c, m0):
    assert c.counter(MEMO) == m0 and "true" not in c.last_kernel(1) and c.last_kernel(1).startswith("k_decompress")


@pytest.mark.parametrize("ntiles", SIZES)
def test_remainder_block_takes_the_classic_path(ctx, ntiles):
    n = ntiles * TILE + 37
    x, c, ref = case(n)
    m0 = ctx.counter(MEMO)
    out, info = ctx.compress(_dev(ctx, x), EB, H.EC)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    _expect_classic(ctx, m0)
    assert _same(rec, ref)


@pytest.mark.parametrize("ntiles", SIZES)
def test_fp32_takes_the_classic_path(ctx, ntiles):
    n = ntiles * TILE
    x, c, ref = case(n, np.float32)
    m0 = ctx.counter(MEMO)
    out, info = ctx.compress(_dev(ctx, x), EB, H.EC)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float32), EB, info.sf, H.EC).cpu().numpy()
    _expect_classic(ctx, m0)
    assert _same(rec, ref)


@pytest.mark.parametrize("ntiles", SIZES)
def test_qt_takes_the_classic_path(ctx, ntiles):
    n = ntiles * TILE
    x, c, ref = case(n, np.float64, O.QT)
    m0 = ctx.counter(MEMO)
    out, info = ctx.compress(_dev(ctx, x), EB, H.QT)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.QT, qtable=np.array(info.qtable[:])).cpu().numpy()
    _expect_classic(ctx, m0)
    assert _same(rec, ref)


@pytest.mark.parametrize("ntiles", SIZES)
def test_another_ac_count_or_other_buffers_take_the_classic_path(ctx, ntiles):
    n = ntiles * TILE
    x, c, ref = case(n)
    m0 = ctx.counter(MEMO)
    out, info = ctx.compress(_dev(ctx, x), EB, H.EC)
    # (AC_exact's buffer holds n floats: one more than the stream needs is a valid, different ac_count)
    rec = ctx.decompress(out, info.cnt + 1, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    _expect_classic(ctx, m0)
    assert _same(rec, ref)
    for moved in ("bin_index", "dc", "ac_exact"):         # any one stream somewhere else
        other = dict(out)
        other[moved] = out[moved].clone()
        rec = ctx.decompress(other, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
        _expect_classic(ctx, m0)
        assert _same(rec, ref)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()      # (and the memo still stands)
    assert ctx.counter(MEMO) == m0 + 1 and _same(rec, ref)


@pytest.mark.parametrize("ntiles", SIZES)
def test_knob_off_and_no_mailbox_take_the_classic_path(ctx, classic, ntiles):
    n = ntiles * TILE
    x, c, ref = case(n)
    nobox = _make({"DCTZHIP_HANDOFF": "0"})
    try:
        for cx in (classic, nobox):
            m0 = cx.counter(MEMO)
            out, info = cx.compress(_dev(cx, x), EB, H.EC)
            rec = cx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
            _expect_classic(cx, m0)
            assert _same(rec, ref)
    finally:
        nobox.close()
    m0 = ctx.counter(MEMO)
    ctx.set_decode_memo(False)
    try:
        out, info = ctx.compress(_dev(ctx, x), EB, H.EC)
        rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
        _expect_classic(ctx, m0)
        assert _same(rec, ref)
    finally:
        ctx.set_decode_memo(True)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()      # (the knob is all that kept it off)
    assert ctx.counter(MEMO) == m0 + 1 and _same(rec, ref)


# ---- 5. invalidation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", SIZES)
@pytest.mark.parametrize("between", ["compress_b", "batch", "set_stream"])
def test_what_rewrites_the_tables_drops_the_memo(ctx, ntiles, between):
    n = ntiles * TILE
    x, c, ref = case(n)
    xd = _dev(ctx, x)
    out, info = ctx.compress(xd, EB, H.EC)
    if between == "compress_b":
        xb, cb, refb = case(3 * TILE + 37)
        outb, infob = ctx.compress(_dev(ctx, xb), EB, H.EC)
    elif between == "batch":
        xs = [_dev(ctx, field(2 * TILE, seed=5)), _dev(ctx, field(TILE + 64 * 3, seed=6))]
        ctx.compress_batch(xs, [EB, EB], H.EC)
    else:
        ctx._bind_stream()
        assert ctx.lib.dctzhip_set_stream(ctx.h, C.c_void_p(ctx._bound)) == 0      # (the same stream again: the call itself drops it)
    m0 = ctx.counter(MEMO)
    rec = ctx.decompress(out, info.cnt, n, _tdt(np.float64), EB, info.sf, H.EC).cpu().numpy()
    _expect_classic(ctx, m0)
    assert _same(rec, ref)
