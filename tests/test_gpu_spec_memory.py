"""The sf guess from the last verified statistics of the same input (include/dctz_hip.h: dctzhip_set_spec_memory;
DESIGN.md sections 3.4 and 3.6).

A speculative compress call on a (buffer, length, element type) that the last calls compressed with one verified scaling
factor takes its guess from their true statistics: no sample, no launch in front of k_compress, and the control block is the
context's other one, zeroed by the last call's k_compact_ac.  Checked here: which calls sample and which remember (debug
counters 18 / 19), that every result is bit for bit the oracle's (FAST) whichever way the guess came about, that a wrong
remembered guess is found and paid for like a wrong sample and backs the input off, what makes a key, the knobs, a
control block that must be clean (QT), and the paths next to it (decode memo, batch, DCTZHIP_HANDOFF=0, profiling).

All on the chain of kernels with the speculation threshold lowered, as spec_ctx in test_gpu_parity.py; sizes 2^20 and
2^20 + 64 * 7 + 40 (a remainder block)."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

EB = 1e-3
SIZES = [1 << 20, (1 << 20) + 64 * 7 + 40]
DTYPES = [np.float64, np.float32]
SPEC_HIT, SPEC_MISS, MEMO, HIST_HIT, HIST_MISS = 6, 7, 16, 18, 19    # dctzhip_debug_counter
NEED = 2                                # verified sampled calls before an input is remembered (dctz_spec_memory.h: NEED_FIRST)
COOLDOWN = 8                            # calls on the full statistics pass after a wrong guess


def _make(env=None):
    import dctz_amd
    env = env or {}
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
    c.set_speculation(True, 1 << 18)
    c.set_one_launch(False)
    return c


@pytest.fixture()
def ctx():
    c = _make()
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)      # (a copy: the cached fields are read-only)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _field(n, dtype, kind="A"):
    """A: smooth + noise, max|x| about 50.  B, C: the same decade without the noise, at about 0.75 and 0.37 of the
    amplitude -- markedly smaller coefficients out of range at every position that has any.  Never modified: callers copy."""
    if kind == "A":
        x = W.ragged(n, dtype, scale=37.0)
    else:
        t = np.arange(n) / 97.0
        x = ((27.5 if kind == "B" else 13.75) * (np.sin(t) + 0.3 * np.cos(5.1 * t))).astype(dtype)
    x.setflags(write=False)
    return x


_ORACLE = {}


def _oracle(x, mode, key=None):
    """O.compress(x, EB, mode, FAST); computed once per key for the fields above."""
    if key is None:
        return O.compress(x, EB, mode, O.FAST)
    k = key + (mode,)
    if k not in _ORACLE:
        _ORACLE[k] = O.compress(x, EB, mode, O.FAST)
    return _ORACLE[k]


def _check(x, mode, out, info, c):
    assert info.sf == c.sf and info.cnt == c.cnt
    assert info.max_abs == float(np.abs(x).max()) and info.min_abs == float(np.abs(x).min())
    assert np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)
    assert _same(out["dc"].cpu().numpy(), c.dc)
    assert _same(out["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact)
    if mode == O.QT:
        assert _same(np.array(info.qtable[:], dtype=x.dtype), c.qtable)
        assert _same(np.array(info.qtable_raw[:], dtype=x.dtype), c.qtable_raw)


def _streak(ctx, xd, out, mode=O.EC, calls=NEED + 1):
    """NEED sampled calls, then remembered ones: returns the infos; the hit counter has moved calls - NEED times."""
    h0 = ctx.counter(HIST_HIT)
    infos = []
    for i in range(calls):
        _, info = ctx.compress(xd, EB, mode, out=out)
        assert info.flags == H.INFO_STATS_FUSED, i
        assert ctx.counter(HIST_HIT) - h0 == max(0, i + 1 - NEED), i
        infos.append(info)
    return infos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [O.EC, O.QT])
@pytest.mark.parametrize("n", SIZES)
def test_hit_after_a_streak_is_bit_exact(ctx, dtype, mode, n):
    x = _field(n, dtype)
    c = _oracle(x, mode, (n, dtype, "A"))
    xd = _dev(ctx, x)
    first = None
    for i in range(5):
        out, info = ctx.compress(xd, EB, mode)       # (fresh outputs per call: compared across the calls below)
        assert info.flags == H.INFO_STATS_FUSED, i
        assert ctx.counter(HIST_HIT) == max(0, i + 1 - NEED), i
        _check(x, mode, out, info, c)
        got = (out["bin_index"].cpu().numpy(), out["dc"].cpu().numpy(), out["ac_exact"][:info.cnt].cpu().numpy(), info.cnt, info.sf,
               info.max_abs, info.min_abs)
        if first is None:
            first = got
        else:
            assert all(_same(a, b) for a, b in zip(got[:3], first[:3])) and got[3:] == first[3:], i
    assert ctx.counter(HIST_MISS) == 0 and ctx.counter(SPEC_MISS) == 0 and ctx.counter(SPEC_HIT) == 5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_decade_change_is_found_and_backs_the_input_off(ctx, dtype, n):
    xd = _dev(ctx, _field(n, dtype))
    out = ctx.alloc_outputs(n, xd.dtype)
    _streak(ctx, xd, out)
    xd.mul_(100.0)                                   # the same buffer, two decades up
    y = xd.cpu().numpy()
    c = _oracle(y, O.EC)
    h0, m0 = ctx.counter(HIST_HIT), ctx.counter(HIST_MISS)
    _, info = ctx.compress(xd, EB, O.EC, out=out)
    assert info.flags == H.INFO_RESPUN
    assert ctx.counter(HIST_MISS) == m0 + 1 and ctx.counter(HIST_HIT) == h0
    _check(y, O.EC, out, info, c)
    assert c.sf == 100.0 * _oracle(_field(n, dtype), O.EC, (n, dtype, "A")).sf
    for i in range(COOLDOWN):                        # the cool-down of any wrong guess
        _, info = ctx.compress(xd, EB, O.EC, out=out)
        assert info.flags == 0, i
    for i in range(2 * NEED + 2):                    # need is doubled: that many sampled calls verify before the input is remembered again
        _, info = ctx.compress(xd, EB, O.EC, out=out)
        assert info.flags == H.INFO_STATS_FUSED, i
        assert ctx.counter(HIST_HIT) - h0 == max(0, i + 1 - 2 * NEED), i
    _check(y, O.EC, out, info, c)
    assert ctx.counter(HIST_MISS) == m0 + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_window_violation_is_found(ctx, dtype, n):
    """The remembered min|x| proved FastDiv's window for every element; an exact zero and a value far below the window
    written into the buffer afterwards must send the call round again."""
    x = np.array(_field(n, dtype))
    x[x == 0] = 1.0
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    _streak(ctx, xd, out)
    x[12345] = 0.0
    x[n - 3] = np.finfo(dtype).tiny * 4
    xd.copy_(_dev(ctx, x))
    m0 = ctx.counter(HIST_MISS)
    _, info = ctx.compress(xd, EB, O.EC, out=out)
    assert info.flags == H.INFO_RESPUN and ctx.counter(HIST_MISS) == m0 + 1
    _check(x, O.EC, out, info, _oracle(x, O.EC))


@pytest.mark.parametrize("n", SIZES)
def test_keys(ctx, n):
    """Another buffer, another length, another element type: not the remembered input."""
    import torch
    x = _field(n, np.float64)
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    _streak(ctx, xd, out)
    h = ctx.counter(HIST_HIT)
    x2 = _dev(ctx, x)                                # (xd is alive: another address)
    assert x2.data_ptr() != xd.data_ptr()
    _, info = ctx.compress(x2, EB, O.EC, out=out)
    assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h
    _, info = ctx.compress(xd[:n - 64], EB, O.EC, out=out)
    assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h
    xf = xd.view(torch.float32)[:n]                  # the same address and length, fp32 (over the first half of xd's bytes)
    xf.copy_(_dev(ctx, _field(n, np.float32)))
    assert xf.data_ptr() == xd.data_ptr()
    outf = ctx.alloc_outputs(n, xf.dtype)
    _, info = ctx.compress(xf, EB, O.EC, out=outf)
    assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h
    _check(_field(n, np.float32), O.EC, outf, info, _oracle(_field(n, np.float32), O.EC, (n, np.float32, "A")))
    assert ctx.counter(HIST_MISS) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_knobs(ctx, dtype, n):
    x = _field(n, dtype)
    c = _oracle(x, O.EC, (n, dtype, "A"))
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    ctx.set_spec_memory(False)
    for i in range(NEED + 2):                        # every call samples
        _, info = ctx.compress(xd, EB, O.EC, out=out)
        assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == 0
    _check(x, O.EC, out, info, c)
    assert ctx.counter(SPEC_HIT) == NEED + 2
    ctx.set_spec_memory(True)
    _streak(ctx, xd, out)
    ctx.set_speculation(False)                       # neither kind of guess, and what was remembered is gone
    h, s = ctx.counter(HIST_HIT), ctx.counter(SPEC_HIT)
    for i in range(2):
        _, info = ctx.compress(xd, EB, O.EC, out=out)
        assert info.flags == 0
    _check(x, O.EC, out, info, c)
    assert ctx.counter(HIST_HIT) == h and ctx.counter(SPEC_HIT) == s
    ctx.set_speculation(True)
    _streak(ctx, xd, out)                            # (a streak from the start: the table was cleared)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_qt_table_on_a_remembered_call_is_this_calls(ctx, dtype, n):
    """QT gathers the per-position maxima with atomicMax into the control block: one that was not zero would show up
    as the LARGER maxima of an earlier call.  Two remembered calls in a row (one on each of the context's two blocks),
    each on data with markedly smaller maxima than the call before."""
    a = _field(n, dtype)
    xd = _dev(ctx, a)
    out = ctx.alloc_outputs(n, xd.dtype)
    infos = _streak(ctx, xd, out, O.QT)
    ca = _oracle(a, O.QT, (n, dtype, "A"))
    _check(a, O.QT, out, infos[-1], ca)
    prev = ca
    for kind in ("B", "C"):
        b = _field(n, dtype, kind)
        cb = _oracle(b, O.QT, (n, dtype, kind))
        assert cb.sf == ca.sf
        # (the fields do what they are for: maxima left behind by the call before would be seen in the table)
        assert np.all(cb.qtable_raw[1:] <= prev.qtable_raw[1:]) and np.sum(cb.qtable_raw[1:] < 0.75 * prev.qtable_raw[1:]) >= 4
        assert not np.array_equal(cb.qtable, prev.qtable)
        xd.copy_(_dev(ctx, b))
        h = ctx.counter(HIST_HIT)
        _, info = ctx.compress(xd, EB, O.QT, out=out)
        assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h + 1
        _check(b, O.QT, out, info, cb)
        prev = cb


@pytest.mark.parametrize("n", SIZES)
def test_memo_decode_after_a_remembered_call(ctx, n):
    """fp64 EC only: the memo decoder exists for that combination alone, and only for n a multiple of 64 (dctz_shim.hip,
    decompress_impl) -- so no fp32 / QT half here.  At 2^20 the decode behind a remembered call takes the memo (counter
    16 moves); at the size with a remainder block it must NOT (counter 16 stays) and decodes the classic way.  Bit-exact
    both times."""
    import torch
    x = _field(n, np.float64)
    c = _oracle(x, O.EC, (n, np.float64, "A"))
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    infos = _streak(ctx, xd, out, calls=NEED + 2)
    m = ctx.counter(MEMO)
    r = ctx.decompress(out, infos[-1].cnt, n, torch.float64, EB, infos[-1].sf, O.EC)
    assert ctx.counter(MEMO) == m + (1 if n % 64 == 0 else 0)
    assert _same(r.cpu().numpy(), O.decompress(c, O.FAST))
    # ... and the call after the decode (which used the call's control block) is a remembered one again, exact
    h = ctx.counter(HIST_HIT)
    _, info = ctx.compress(xd, EB, O.EC, out=out)
    assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h + 1
    _check(x, O.EC, out, info, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [O.EC, O.QT])
@pytest.mark.parametrize("n", SIZES)
def test_other_calls_in_between(ctx, mode, n, dtype):
    """A batch call and the compress of another (small: plain statistics) array between two remembered calls: both use
    control blocks of the context; the next remembered call's results are the oracle's."""
    x = _field(n, dtype)
    c = _oracle(x, mode, (n, dtype, "A"))
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    _streak(ctx, xd, out, mode)
    small = W.ragged(64 * 300 + 41, dtype, scale=370.0)
    ys = [W.ragged(64 * 90 + 33, np.float32, scale=5.0), W.ragged(64 * 50, np.float64, scale=2.0)]
    for between in ("single", "batch"):
        if between == "single":
            o2, i2 = ctx.compress(_dev(ctx, small), EB, mode)
            _check(small, mode, o2, i2, _oracle(small, mode, ("small", dtype)))
        else:
            outs, infos, _ = ctx.compress_batch([_dev(ctx, y) for y in ys], [EB, EB], mode)
            for y, o_, i_ in zip(ys, outs, infos):
                cy = _oracle(y, mode, ("batch", y.size))
                assert i_.sf == cy.sf and i_.cnt == cy.cnt and np.array_equal(o_["bin_index"].cpu().numpy(), cy.bin_index)
        h = ctx.counter(HIST_HIT)
        _, info = ctx.compress(xd, EB, mode, out=out)
        assert info.flags == H.INFO_STATS_FUSED and ctx.counter(HIST_HIT) == h + 1, between
        _check(x, mode, out, info, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [O.EC, O.QT])
@pytest.mark.parametrize("n", SIZES)
def test_without_the_mailbox(mode, n, dtype):
    """DCTZHIP_HANDOFF=0: no hand-off workgroup, so no zeroed second block; whichever way the guess comes about, the
    results are the oracle's."""
    ctx = _make({"DCTZHIP_HANDOFF": "0"})
    try:
        x = _field(n, dtype)
        c = _oracle(x, mode, (n, dtype, "A"))
        xd = _dev(ctx, x)
        out = ctx.alloc_outputs(n, xd.dtype)
        for i in range(NEED + 2):
            _, info = ctx.compress(xd, EB, mode, out=out)
            assert info.flags == H.INFO_STATS_FUSED, i
            _check(x, mode, out, info, c)
        assert ctx.counter(SPEC_HIT) == NEED + 2 and ctx.counter(SPEC_MISS) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_timings_on_a_remembered_call(ctx, n, dtype):
    x = _field(n, dtype)
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    ctx.set_profiling(True)
    infos = _streak(ctx, xd, out)
    t = ctx.timings()
    assert set(t) == {"stats_ms", "main_ms", "tail_ms", "total_ms"}
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    assert t["main_ms"] > 0.0 and t["total_ms"] >= t["main_ms"]
    assert abs(t["total_ms"] - (t["stats_ms"] + t["main_ms"] + t["tail_ms"])) <= 1e-3 * max(1.0, t["total_ms"])
    _check(x, O.EC, out, infos[-1], _oracle(x, O.EC, (n, dtype, "A")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_input_the_library_owns_is_not_remembered(ctx, dtype):
    """compress_masked without `filled` compresses the context's own filled copy: every masked array of one size would
    share that key.  Such calls sample every time and leave the table alone; results are the oracle's for the filled array."""
    n = SIZES[0]
    x = np.array(_field(n, dtype))
    x[777] = np.nan
    xd = _dev(ctx, x)
    out = ctx.alloc_outputs(n, xd.dtype)
    for i in range(NEED + 2):
        _, info, _, count = ctx.compress_masked(xd, EB, H.MISS_NAN, out=out)
        assert count == 1 and info.flags == H.INFO_STATS_FUSED, i
        assert ctx.counter(HIST_HIT) == 0 and ctx.counter(HIST_MISS) == 0, i
    assert ctx.counter(SPEC_HIT) == NEED + 2
    # the same call with the caller's own buffer for the filled copy IS remembered, and gives the same streams
    filled = xd.clone()
    ref = {k: v.clone() for k, v in out.items()}
    for i in range(NEED + 1):
        _, info2, _, _ = ctx.compress_masked(xd, EB, H.MISS_NAN, out=out, filled=filled)
        assert info2.flags == H.INFO_STATS_FUSED, i
    assert ctx.counter(HIST_HIT) == 1
    assert info2.cnt == info.cnt and info2.sf == info.sf
    assert all(_same(out[k][:(info.cnt if k == "ac_exact" else None)].cpu().numpy(), ref[k][:(info.cnt if k == "ac_exact" else None)].cpu().numpy()) for k in out)
    f = filled.cpu().numpy()
    _check(f, O.EC, out, info2, _oracle(f, O.EC))
