"""Coefficients at the bin edges on every path that bins them, bit for bit against the oracle (FAST).

The arrays of tests/bin_edge_cases.py hold coefficients ON range_max, ON range_min, one ulp outside either, on an interior
bin edge and -- where the bound has one -- in the one-ulp strip above range_max where bin_value<T, SAFE = false> and the
reference's range test disagree (tests/test_bin_edge_cases_cpu.py counts them and shows that a kernel without the range test
would differ there and only there).  Every path that bins is run on them: the one-launch kernel, the chain (k_compress, with
fused statistics too), the scaled copy out of place and in place, k_compress_eo with lists and with single-pass placement,
the batch kernels (items with different bounds in one call, and hundreds of short last blocks through bin_short), the tiled
kernels, both probes, and contexts created under DCTZHIP_FASTDIV=0 / =1 and DCTZHIP_DEVICE_SF=0.  Which of the three binning
variants a call ran is read from dctzhip_debug_counter 20 and must be what bin_edge_cases.classify predicts, so that no case
silently runs another variant than the one it names."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import bin_edge_cases as B
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

VARIANT = 20                            # dctzhip_debug_counter: fast_sf | fast_bw << 8 of the last verified pass
MODES = [O.EC, O.QT]
FLAT = B.select("flat")
TILED = B.select("tiled")
SHORT = B.select("short")
KNOBS = {"fastdiv0": ({"DCTZHIP_FASTDIV": "0"}, 0), "fastdiv1": ({"DCTZHIP_FASTDIV": "1"}, 1), "hostsf": ({"DCTZHIP_DEVICE_SF": "0"}, 2)}

_CTX = {}


def _make(env):
    """A context created under `env` (the knobs are read when the context is created), as tests/test_gpu_spec_memory.py::_make."""
    import dctz_amd
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return dctz_amd.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx(path, knob=None):
    """path: "one" (default context), "chain" (set_one_launch(False)), "spec" (chain, speculation from 2^18 elements)."""
    key = (path, knob)
    if key not in _CTX:
        c = _make(KNOBS[knob][0] if knob else {})
        if path != "one":
            c.set_one_launch(False)
        if path == "spec":
            c.set_speculation(True, 1 << 18)
            c.set_spec_memory(False)    # every call samples: the sets follow each other through one buffer with sf 1 and 100
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)      # (a copy: the cached sets are read-only)


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_streams(out, info, c, mode, dtype, raw_from=0):
    assert info.sf == c.sf and info.cnt == c.cnt, (info.sf, c.sf, info.cnt, c.cnt)
    got = out["bin_index"].cpu().numpy()
    bad = np.flatnonzero(got != c.bin_index)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], c.bin_index[bad[:8]])
    assert _same(out["dc"].cpu().numpy(), c.dc)
    assert _same(out["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact)
    if mode == O.QT:
        assert _same(np.array(info.qtable[:], dtype=dtype), c.qtable)
        assert _same(np.array(info.qtable_raw[raw_from:], dtype=dtype), c.qtable_raw[raw_from:])


@functools.lru_cache(maxsize=None)
def _decoded(case, mode, i=0):
    c = case.oracle(mode)[i]
    r = O.decompress_nd(c, case.arrays()[i].shape, O.FAST) if case.kind == "tiled" else O.decompress(c, O.FAST)
    r.setflags(write=False)
    return r


def _check_decode(ctx, out, info, case, mode):
    x = case.arrays()[0]
    q = np.array(info.qtable[:]) if mode == O.QT else None
    if case.kind == "tiled":
        r = ctx.decompress_nd(out, info.cnt, x.shape, _tdt(case.dtype), case.eb, info.sf, mode, qtable=q)
    else:
        r = ctx.decompress(out, info.cnt, x.size, _tdt(case.dtype), case.eb, info.sf, mode, qtable=q)
    assert _same(r.cpu().numpy(), _decoded(case, mode))


def _flat(ctx, case, mode, fastdiv=2, **kw):
    x = case.arrays()[0]
    out, info = ctx.compress(_dev(ctx, x), case.eb, mode, **kw)
    _check_streams(out, info, case.oracle(mode)[0], mode, case.dtype)
    assert ctx.counter(VARIANT) == B.variant(x, case.eb, case.dtype, fastdiv), (hex(ctx.counter(VARIANT)), case.name)
    return out, info


# ---- one launch, the chain, the chain with fused statistics ---------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["one", "chain", "spec"])
@pytest.mark.parametrize("case", FLAT, ids=repr)
def test_flat(case, path, mode):
    ctx = _ctx(path)
    out, info = _flat(ctx, case, mode)
    assert bool(info.flags & H.INFO_ONE_LAUNCH) == (path == "one")      # (about 100 tiles: resident at once)
    if path == "spec":
        assert info.flags & H.INFO_STATS_FUSED and not info.flags & H.INFO_RESPUN
    if path == "chain":
        assert not info.flags & (H.INFO_STATS_FUSED | H.INFO_SPLIT)
    _check_decode(ctx, out, info, case, mode)


def test_every_variant_is_reached_by_a_bound():
    """fast_bw 3, 1 and (fp32) 0 from the bounds alone; the sets in FastDiv's numerator window throughout (fast_sf 2)."""
    want = {np.dtype(np.float32): {0x302, 0x102, 0x002}, np.dtype(np.float64): {0x302, 0x102}}
    for dtype, v in want.items():
        assert {B.variant(c.arrays()[0], c.eb, c.dtype) for c in FLAT if c.dtype == dtype} == v


# ---- the scaled copy: x / sf runs through FastDiv first (sf = 100) --------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["copy-one", "copy-chain", "in-place"])
@pytest.mark.parametrize("case", B.select("flat", tag="sf100"), ids=repr)
def test_scaled_copy(case, how, mode):
    import torch
    ctx = _ctx("chain" if how == "copy-chain" else "one")
    x = case.arrays()[0]
    c = case.oracle(mode)[0]
    assert c.sf == 100.0
    xd = _dev(ctx, x)
    scaled = xd if how == "in-place" else torch.zeros_like(xd)
    out, info = ctx.compress(xd, case.eb, mode, scaled=scaled)
    _check_streams(out, info, c, mode, case.dtype)
    assert ctx.counter(VARIANT) == B.variant(x, case.eb, case.dtype)
    assert bool(info.flags & H.INFO_ONE_LAUNCH) == (how == "copy-one")    # (in place: the chain, on verified statistics)
    assert _same(scaled.cpu().numpy(), c.scaled)
    if how != "in-place":
        assert _same(xd.cpu().numpy(), x)
    _check_decode(ctx, out, info, case, mode)


# ---- k_compress_eo: lists, and single-pass placement ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("case", B.select("flat", np.float64), ids=repr)
def test_split_kernel(case, split, mode):
    ctx = _ctx("chain")
    ctx.set_split(split)
    try:
        out, info = _flat(ctx, case, mode)
    finally:
        ctx.set_split(0)
    assert info.flags & H.INFO_SPLIT and not info.flags & H.INFO_ONE_LAUNCH
    assert bool(info.flags & H.INFO_SINGLE_PASS) == (split == 3 and mode == O.EC)
    _check_decode(ctx, out, info, case, mode)


# ---- batches: items with different bounds in one call; hundreds of short last blocks --------------------------------------
def _batch_items(dtype):
    """(case, index of the array in the case) for every item: the flat sets at the strip, the bit-1 and (fp32) the
    out-of-window bound, then every short-block array."""
    flat = [c for c in FLAT if c.dtype == np.dtype(dtype) and "sf1-" in c.name + "-"]
    return [(c, 0) for c in flat] + [(c, i) for c in SHORT if c.dtype == np.dtype(dtype) for i in range(len(c.arrays()))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["one", "chain"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch(dtype, path, mode):
    import torch
    ctx = _ctx(path)
    items = _batch_items(dtype)
    ebs = [c.eb for c, _ in items]
    assert {B.classify(e, dtype) for e in ebs} == ({0, 1, 3} if dtype == np.float32 else {1, 3})
    xs = [c.arrays()[i] for c, i in items]
    # one upload, one set of output buffers: every item at a multiple of 128 elements (16-byte aligned in every stream)
    offs = np.concatenate([[0], np.cumsum([-(-x.size // 128) * 128 for x in xs])]).astype(np.int64)
    host = np.zeros(offs[-1], dtype)
    for x, o in zip(xs, offs):
        host[o:o + x.size] = x
    big = _dev(ctx, host)
    bins = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=ctx.device)
    dcs = torch.zeros(int(offs[-1]), dtype=torch.float32, device=ctx.device)
    acs = torch.zeros(int(offs[-1]), dtype=torch.float32, device=ctx.device)
    xd = [big[o:o + x.size] for x, o in zip(xs, offs)]
    outs = [{"bin_index": bins[o:o + x.size], "dc": dcs[o:o + (x.size + 63) // 64], "ac_exact": acs[o:o + x.size]} for x, o in zip(xs, offs)]
    _, infos, _ = ctx.compress_batch(xd, ebs, mode, outs=outs)
    hb, hd, ha = bins.cpu().numpy(), dcs.cpu().numpy(), acs.cpu().numpy()
    short_blocks = 0
    for (case, i), x, o, info in zip(items, xs, offs, infos):
        c = case.oracle(mode)[i]
        assert info.sf == c.sf and info.cnt == c.cnt, (case.name, i, info.cnt, c.cnt)
        assert np.array_equal(hb[o:o + x.size], c.bin_index), (case.name, i)
        assert _same(hd[o:o + c.dc.size], c.dc) and _same(ha[o:o + c.cnt], c.ac_exact), (case.name, i)
        if mode == O.QT:
            assert _same(np.array(info.qtable[:], dtype=dtype), c.qtable)
            assert _same(np.array(info.qtable_raw[1:], dtype=dtype), c.qtable_raw[1:])
        short_blocks += x.size % 64 != 0
    assert short_blocks >= 1000                        # bin_short, many times in one call
    dsts, status, _ = ctx.decompress_batch(outs, [f.cnt for f in infos], [x.size for x in xs], [_tdt(dtype)] * len(xs), ebs,
                                          [f.sf for f in infos], mode, qtables=[np.array(f.qtable[:]) for f in infos])
    assert not any(status)
    for (case, i), r in zip(items[:8] + items[8::37], dsts[:8] + dsts[8::37]):
        assert _same(r.cpu().numpy(), _decoded(case, mode, i)), (case.name, i)


# ---- arrays compressed in 8 x 8 and 4 x 4 x 4 tiles -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", TILED, ids=repr)
def test_tiled(case, mode):
    ctx = _ctx("one")
    x = case.arrays()[0]
    out, info = ctx.compress_nd(_dev(ctx, x), case.eb, mode)
    _check_streams(out, info, case.oracle(mode)[0], mode, case.dtype)
    assert ctx.counter(VARIANT) == B.variant(x, case.eb, case.dtype)
    _check_decode(ctx, out, info, case, mode)


# ---- the probes: one call lists strip, bit-1 and (fp32) out-of-window bounds together ---------------------------------------
@functools.lru_cache(maxsize=None)
def _cnt(case, eb):
    f = O.compress_nd if case.kind == "tiled" else O.compress
    return f(case.arrays()[0], eb, O.EC, O.FAST).cnt


def _probe_bounds(dtype):
    b = B.BOUNDS[np.dtype(dtype)]
    ebs = [b["strip"], b["bit1"], 1e-6, b["strip"]] + ([b["plain"], b["strip"]] if "plain" in b else [3.7e-5])
    assert {B.classify(e, dtype) for e in ebs} >= {1, 3}
    return ebs


@pytest.mark.parametrize("case", [c for c in FLAT + TILED if "plain" not in c.name], ids=repr)
def test_probe_counts(case):
    ctx = _ctx("one")
    ebs = _probe_bounds(case.dtype)
    xd = _dev(ctx, case.arrays()[0])
    pts, _ = ctx.rd_probe_nd(xd, ebs) if case.kind == "tiled" else ctx.rd_probe(xd, ebs)
    assert [p["cnt"] for p in pts] == [_cnt(case, e) for e in ebs], case.name
    assert case.eb in ebs                             # (the bound whose edges the data sits on is among them)


# ---- contexts under the documented knobs: plain division, FastDiv level 1, the host's choice of sf --------------------------
@functools.lru_cache(maxsize=None)
def _ragged(dtype):
    x = W.ragged(4096 * 9 + 64 * 5 + 40, dtype, scale=37.0)      # a short last block; exceptions everywhere at eb 1e-3
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("path", ["one", "chain"])
@pytest.mark.parametrize("case", FLAT, ids=repr)
@pytest.mark.parametrize("knob", list(KNOBS))
def test_knob_contexts(knob, case, path):
    ctx = _ctx(path, knob)
    level = KNOBS[knob][1]
    for mode in MODES:
        out, info = _flat(ctx, case, mode, fastdiv=level)
        # (DCTZHIP_DEVICE_SF=0: the one-launch kernel, which chooses sf itself, declines)
        assert bool(info.flags & H.INFO_ONE_LAUNCH) == (path == "one" and knob != "hostsf")
        v = ctx.counter(VARIANT)
        if level == 0:
            assert v == 0
        elif level == 1:
            assert (v & 0xff) <= 1 and (v >> 8) <= 1
    _check_decode(ctx, out, info, case, MODES[-1])


@pytest.mark.parametrize("path", ["one", "chain"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("knob", list(KNOBS))
def test_knob_contexts_ragged(knob, dtype, path):
    ctx = _ctx(path, knob)
    x = _ragged(dtype)
    for mode in MODES:
        for eb in B.BOUNDS[np.dtype(dtype)].values():
            c = O.compress(x, eb, mode, O.FAST)
            out, info = ctx.compress(_dev(ctx, x), eb, mode)
            _check_streams(out, info, c, mode, dtype)
            assert ctx.counter(VARIANT) == B.variant(x, eb, dtype, KNOBS[knob][1])
            r = ctx.decompress(out, info.cnt, x.size, _tdt(dtype), eb, info.sf, mode, qtable=np.array(info.qtable[:]))
            assert _same(r.cpu().numpy(), O.decompress(c, O.FAST))
