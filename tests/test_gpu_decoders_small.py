"""Every decoder on the same streams, each held to the oracle bit for bit.

The de-quantise step and the short last block are written once (dctz_kernel_common.h) and called from four decoders; by
default a call reaches only one of them (the one-launch kernel for arrays this small, k_decompress_il for fp64 EC on the
chain, k_decompress for the rest), so a helper that one call site uses wrongly could hide behind the default path.  Here
the oracle's streams of a few small arrays go through the one-launch kernel, both chain kernels (forced by the
environment, the kernel's name checked), the range decoder over [0, n) and the batch entry point.

Shapes, the smallest that reach every branch: a partial last tile with an odd short block (length-2l transform), an even
short block, and no short block at all (the chain then hands over early).  Data: sparse exceptions (ragged, eb 1e-3: the
tile's coefficients staged one tile ahead) and dense ones (heavy tails, eb 1e-6: more than 2048 per tile, beyond the
staging capacity of both element types)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE = 4096
NS = (3 * TILE + 9 * 64 + 21, 2 * TILE + 40, TILE)
KINDS = {"sparse": 1e-3, "dense": 1e-6}
# decoder -> (environment of its context, the kernel dctzhip_debug_last_kernel must name; None: not a whole-array path)
DECODERS = {
    "one": ({}, "k_decompress_one<{t}, {m}>"),
    "chain": ({"DCTZHIP_ONE": "0", "DCTZHIP_DEC_IL": "0"}, "k_decompress<{t}, {m}, {ph}, 0>"),
    "chain_il": ({"DCTZHIP_ONE": "0", "DCTZHIP_DEC_IL": "2"}, "k_decompress_il<{t}, {m}, {ph}>"),
    "range": ({}, None),
    "batch": ({}, None),
}


def _input(n, kind, dtype):
    base = W.ragged(n, np.float64, scale=37.0)
    if kind == "dense":                            # heavy tails: most coefficients out of range
        base = base + 200.0 * np.random.default_rng(99).standard_cauchy(n).clip(-1e3, 1e3)
    return base.astype(dtype)


def _tile_counts(bin_index, n):
    """Exact coefficients per tile: bin id 255 at an in-block position j >= 1 (the short block's positions included)."""
    f = (np.asarray(bin_index[:n]) == 255) & (np.arange(n) % 64 != 0)
    return np.add.reduceat(f.astype(np.int64), np.arange(0, n, TILE)), f


_REF = {}


def _reference(n, kind, dtype, mode):
    """(streams of the oracle, its reconstruction) of one case, computed once and never written to; the conditions on the
    input are checked here, on the CPU, before anything of the case runs on the GPU."""
    key = (n, kind, np.dtype(dtype).name, mode)
    if key not in _REF:
        c = O.compress(_input(n, kind, dtype), KINDS[kind], mode, O.FAST)
        per_tile, f = _tile_counts(c.bin_index, n)
        assert int(per_tile.sum()) == c.cnt
        if kind == "dense":
            assert per_tile.max() > 2048, per_tile          # the unstaged branch, for both element types
        else:
            assert ((per_tile >= 1) & (per_tile <= 1024)).any(), per_tile
        if n % 64:
            assert f[n - n % 64:].any(), "the short block has no exact coefficient"
        ref = O.decompress(c, O.FAST)
        ref.setflags(write=False)
        _REF[key] = (c, ref)
    return _REF[key]


def _upload(ctx, c):
    import torch
    out = ctx.alloc_outputs(c.n)
    out["bin_index"].copy_(torch.from_numpy(c.bin_index))
    out["dc"].copy_(torch.from_numpy(c.dc))
    out["ac_exact"][:c.cnt].copy_(torch.from_numpy(c.ac_exact))
    return out


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mode", [O.EC, O.QT], ids=["EC", "QT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("decoder", list(DECODERS))
def test_every_decoder_is_the_oracle_bit_for_bit(decoder, dtype, mode, kind, monkeypatch):
    import torch
    import dctz_amd
    refs = [_reference(n, kind, dtype, mode) for n in NS]
    env, kernel = DECODERS[decoder]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    eb = KINDS[kind]
    ctx = dctz_amd.Context(0)
    try:
        outs = [_upload(ctx, c) for c, _ in refs]
        if decoder == "batch":
            got, status, _ = ctx.decompress_batch(outs, [c.cnt for c, _ in refs], list(NS), [tdt] * len(NS), eb, [c.sf for c, _ in refs],
                                                  mode, qtables=[c.qtable for c, _ in refs])
            assert all(s == 0 for s in status), status
        else:
            got = []
            for n, out, (c, _) in zip(NS, outs, refs):
                if decoder == "range":
                    idx, tot = ctx.ac_index(out, n)
                    assert tot == c.cnt
                    got.append(ctx.decompress_range(out, c.cnt, n, tdt, eb, c.sf, 0, n, idx, mode, qtable=c.qtable))
                else:
                    got.append(ctx.decompress(out, c.cnt, n, tdt, eb, c.sf, mode, qtable=c.qtable))
                    want = kernel.format(t="double" if dtype == np.float64 else "float", m=mode, ph=1 if dtype == np.float64 else 2)
                    assert ctx.last_kernel(1) == want, (n, ctx.last_kernel(1))
        for n, r, (_, ref) in zip(NS, got, refs):
            r = r.cpu().numpy()
            bad = np.flatnonzero(_bits(r) != _bits(ref))
            assert bad.size == 0, f"n = {n}: {bad.size} mismatches, first {bad[:8]} (blocks {np.unique(bad // 64)[:8]})"
    finally:
        ctx.close()
