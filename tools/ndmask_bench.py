#!/usr/bin/env python3
"""The missing-value layer of tiled arrays, measured: one process, the bytes of tools/ndfix_bench.py (the
synthetic fp64 512^3 shard, C4's shard 0) with about a quarter of the elements marked 1e36 in smooth blobs, EC, eb 1e-3, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles, and
  a 8192 x 16384 field in 8 x 8 tiles.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported with min ... max:

  dctzhip_mask_build_nd, out of place    mask, count and the filled copy in another buffer
  dctzhip_mask_build_nd, in place        ... over the input (the holes are put back before the next round, outside the timing)
  dctzhip_mask_build_nd, mask only       d_filled = NULL
  dctzhip_mask_build (flat), out of pl.  the flat kernel over the same buffer: the same traffic, the only call to compare against
  device-to-device copy                  the same array: the floor for the bytes of the out-of-place call
  dctzhip_compress_nd(filled)            the plain tiled call on the filled array
  dctzhip_compress_masked_nd             fill + compress
all through the C ABI on buffers allocated once.  The condition (2-D, where every row of a trip is a whole line): the tiled
out-of-place build's median lies no further above the flat build's median than the flat row's own max - min of this run; for
3-D (64-byte row pieces) the ratio is stated.  One JSON line per array goes to stdout; --out writes the tables as text
(profiles/ndmask_layer.txt)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def holes_of(torch, shape, device):
    """Smooth blobs over the array, about a quarter of it."""
    ax = [torch.arange(d, dtype=torch.float64, device=device) for d in shape]
    if len(shape) == 3:
        zz, yy, xx = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
        f = torch.sin(xx / 41.0 + 0.5) * torch.cos(yy / 29.0) + 0.6 * torch.sin((xx + 2 * yy + 3 * zz) / 67.0) + 0.4 * torch.cos(zz / 23.0)
    else:
        yy, xx = ax[0][:, None], ax[1][None, :]
        f = torch.sin(xx / 41.0 + 0.5) * torch.cos(yy / 29.0) + 0.6 * torch.sin((xx + 2 * yy) / 67.0) + 0.4 * torch.cos(yy / 23.0)
    return f > 0.45


def measure(ctx, x0, shape, a):
    import numpy as np
    import torch
    import dctz_amd
    from dctz_amd import hip as H

    tdt, eb = torch.float64, 1e-3
    nd, n = len(shape), x0.numel()
    holes = holes_of(torch, shape, ctx.device)
    frac = float(holes.double().mean())
    x = x0.clone().reshape(shape)
    x[holes] = 1e36
    del holes
    dims = (C.c_size_t * nd)(*shape)
    miss = H.Missing(H.MISS_VALUE, 1e36, 0.0)
    words = int(ctx.lib.dctzhip_mask_words(n))
    mask = torch.empty(words, dtype=torch.int64, device=ctx.device)
    flat_mask = torch.empty_like(mask)
    filled = torch.empty_like(x)
    flat_filled = torch.empty_like(x)
    work = x.clone()
    copy_dst = torch.empty_like(x)
    out = ctx.alloc_outputs(ctx.nd_blocks(shape) * 64, tdt)
    info, count = H.CompressInfo(), C.c_uint64(0)
    # once through the binding: what the timed calls must reproduce
    want_mask, want_count, want_filled = ctx.mask_build_nd(x, miss)
    ref_out, ref_info = ctx.compress_nd(want_filled, eb, dctz_amd.EC)
    ref_cnt = ref_info.cnt
    plain = ctx.compress_nd(x, eb, dctz_amd.EC)[1]

    def build(src, dst):
        rc = ctx.lib.dctzhip_mask_build_nd(ctx.h, src.data_ptr(), nd, dims, H.F64, C.byref(miss), mask.data_ptr(),
                                           dst.data_ptr() if dst is not None else None, C.byref(count))
        assert rc == H.OK and count.value == want_count, (rc, count.value)

    def build_flat():
        rc = ctx.lib.dctzhip_mask_build(ctx.h, x.data_ptr(), n, H.F64, C.byref(miss), flat_mask.data_ptr(), flat_filled.data_ptr(), C.byref(count))
        assert rc == H.OK and count.value == want_count, (rc, count.value)

    def compress_filled():
        rc = ctx.lib.dctzhip_compress_nd(ctx.h, want_filled.data_ptr(), nd, dims, H.F64, eb, dctz_amd.EC, out["bin_index"].data_ptr(),
                                         out["dc"].data_ptr(), out["ac_exact"].data_ptr(), None, C.byref(info))
        assert rc == H.OK and info.cnt == ref_cnt

    def compress_masked():
        rc = ctx.lib.dctzhip_compress_masked_nd(ctx.h, x.data_ptr(), nd, dims, H.F64, eb, dctz_amd.EC, C.byref(miss), out["bin_index"].data_ptr(),
                                                out["dc"].data_ptr(), out["ac_exact"].data_ptr(), mask.data_ptr(), filled.data_ptr(),
                                                C.byref(info), C.byref(count))
        assert rc == H.OK and info.cnt == ref_cnt and count.value == want_count

    calls = [("mask_build_nd, out of place", lambda: build(x, filled), None),
             ("mask_build_nd, in place", lambda: build(work, work), lambda: work.copy_(x)),
             ("mask_build_nd, mask only", lambda: build(x, None), None),
             ("mask_build (flat), out of pl.", build_flat, None),
             ("device-to-device copy", lambda: copy_dst.copy_(x), None),
             ("compress_nd(filled)", compress_filled, None),
             ("compress_masked_nd", compress_masked, None)]
    ms = {name: [] for name, _, _ in calls}
    for r in range(a.warmup + a.rounds):
        for name, fn, before in calls:
            if before:
                before()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
    # what was timed is the layer
    assert torch.equal(mask, want_mask) and torch.equal(flat_mask, want_mask)
    assert torch.equal(filled.view(torch.int64), want_filled.view(torch.int64)) and torch.equal(work.view(torch.int64), want_filled.view(torch.int64))
    assert torch.equal(out["bin_index"], ref_out["bin_index"]) and info.sf == ref_info.sf
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lo = {k: float(np.min(v)) for k, v in ms.items()}
    hi = {k: float(np.max(v)) for k, v in ms.items()}
    both = (16 * n + n / 8) / 1e9
    gb = {"mask_build_nd, out of place": both, "mask_build_nd, in place": both, "mask_build_nd, mask only": (8 * n + n / 8) / 1e9,
          "mask_build (flat), out of pl.": both, "device-to-device copy": 16 * n / 1e9}
    tiles = "8 x 8" if nd == 2 else "4 x 4 x 4"
    lines = [f"missing-value layer, fp64 {' x '.join(map(str, shape))} in {tiles} tiles, EC eb = {eb}, {want_count} of {n} elements 1e36 in "
             f"smooth blobs ({frac:.3f})",
             f"sf: plain compress_nd {plain.sf:g}, masked {ref_info.sf:g}; exact coefficients: plain {plain.cnt}, masked {ref_cnt}",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds",
             f"{'call':<32}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}{'TB/s':>8}"]
    for name, _, _ in calls:
        g_ = gb.get(name)
        lines.append(f"{name:<32}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}" +
                     (f"{g_:>10.3f}{g_ / med[name]:>8.2f}" if g_ else f"{'':>10}{'':>8}"))
    nd_ms, flat_ms = med["mask_build_nd, out of place"], med["mask_build (flat), out of pl."]
    spread = hi["mask_build (flat), out of pl."] - lo["mask_build (flat), out of pl."]
    verdict = f"tiled / flat build = {nd_ms / flat_ms:.3f}; tiled - flat = {nd_ms - flat_ms:+.4f} ms, the flat row's max - min = {spread:.4f} ms"
    if nd == 2:
        verdict += ": condition " + ("MET" if nd_ms - flat_ms <= spread else "NOT MET")
    lines.append(verdict)
    lines.append(f"compress_masked_nd - compress_nd(filled) = {med['compress_masked_nd'] - med['compress_nd(filled)']:.4f} ms; "
                 f"mask_build_nd out of place / copy = {nd_ms / med['device-to-device copy']:.2f}")
    js = {"what": "ndmask_layer", "shape": list(shape), "missing": want_count, "median_ms": {k: round(v, 4) for k, v in med.items()},
          "tiled_over_flat": round(nd_ms / flat_ms, 4), "flat_spread_ms": round(spread, 4)}
    return "\n".join(lines) + "\n", js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="edge of the cube; the 2-D workload is the same bytes as n^2 / 32 x 32 n")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dctz_amd
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("ndmask_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e = a.n
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    text = ""
    for shape in ((e, e, e), (e * e // 32, 32 * e)):
        t, js = measure(ctx, x, shape, a)
        text += t + "\n"
        sys.stderr.write(t + "\n")
        print(json.dumps(js), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
