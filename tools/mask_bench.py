#!/usr/bin/env python3
"""The missing-value layer, measured: one process, the synthetic fp64 512^3 shard (C4's shard 0) with
about 27 % of it marked 1e36 in smooth blobs, EC, eb 1e-3.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported:

  dctzhip_mask_build, out of place     mask, count and the filled copy in another buffer
  dctzhip_mask_build, in place         ... over the input (the holes are put back before the next round, outside the timing)
  dctzhip_mask_build, mask only        d_filled = NULL
  device-to-device copy                the same array: the floor for the bytes of the out-of-place call
  dctzhip_compress(filled)             the plain call on the filled array
  dctzhip_compress_masked              fill + compress; its difference to the line above is what a fused fill could save at most
  dctzhip_mask_apply, whole array      on a decode of the streams
all through the C ABI on buffers allocated once.  No ratio is fixed in advance.  One JSON line goes to stdout; --out writes the
table as text (profiles/mask_layer.txt)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="edge of the cube")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dctz_amd
    from dctz_amd import hip as H
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("mask_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e, tdt, eb, fill = a.n, torch.float64, 1e-3, -9.96921e36
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    n = x.numel()
    # smooth blobs over the cube, about 27 % of it
    g = torch.arange(e, dtype=tdt, device=ctx.device) * (512.0 / e)
    zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
    holes = ((torch.sin(xx / 41.0 + 0.5) * torch.cos(yy / 29.0) + 0.6 * torch.sin((xx + 2 * yy + 3 * zz) / 67.0)
              + 0.4 * torch.cos(zz / 23.0)) > 0.45).reshape(-1)
    del zz, yy, xx
    frac = float(holes.double().mean())
    x[holes] = 1e36
    miss = H.Missing(H.MISS_VALUE, 1e36, 0.0)
    words = int(ctx.lib.dctzhip_mask_words(n))
    mask = torch.empty(words, dtype=torch.int64, device=ctx.device)
    filled = torch.empty_like(x)
    work = x.clone()
    copy_dst = torch.empty_like(x)
    out = ctx.alloc_outputs(n, tdt)
    info, count = H.CompressInfo(), C.c_uint64(0)
    # once through the binding: what the timed calls must reproduce
    want_mask, want_count, want_filled = ctx.mask_build(x, miss)
    assert want_count == int(holes.sum())
    ref_out, ref_info = ctx.compress(want_filled, eb, dctz_amd.EC)
    ref_cnt = ref_info.cnt
    dec = ctx.decompress(ref_out, ref_cnt, n, tdt, eb, ref_info.sf, dctz_amd.EC)
    plain = ctx.compress(x, eb, dctz_amd.EC)[1]

    def build(src, dst):
        rc = ctx.lib.dctzhip_mask_build(ctx.h, src.data_ptr(), n, H.F64, C.byref(miss), mask.data_ptr(), dst.data_ptr() if dst is not None else None,
                                        C.byref(count))
        assert rc == H.OK and count.value == want_count, (rc, count.value)

    def compress_filled():
        rc = ctx.lib.dctzhip_compress(ctx.h, want_filled.data_ptr(), n, H.F64, eb, dctz_amd.EC, out["bin_index"].data_ptr(), out["dc"].data_ptr(),
                                      out["ac_exact"].data_ptr(), None, None, C.byref(info))
        assert rc == H.OK and info.cnt == ref_cnt

    def compress_masked():
        rc = ctx.lib.dctzhip_compress_masked(ctx.h, x.data_ptr(), n, H.F64, eb, dctz_amd.EC, C.byref(miss), out["bin_index"].data_ptr(),
                                             out["dc"].data_ptr(), out["ac_exact"].data_ptr(), mask.data_ptr(), filled.data_ptr(), C.byref(info),
                                             C.byref(count))
        assert rc == H.OK and info.cnt == ref_cnt and count.value == want_count

    calls = [("mask_build, out of place", lambda: build(x, filled), None),
             ("mask_build, in place", lambda: build(work, work), lambda: work.copy_(x)),
             ("mask_build, mask only", lambda: build(x, None), None),
             ("device-to-device copy", lambda: copy_dst.copy_(x), None),
             ("compress(filled)", compress_filled, None),
             ("compress_masked", compress_masked, None),
             ("mask_apply, whole array", lambda: ctx.mask_apply(mask, n, fill, dec), None)]
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
    assert torch.equal(mask, want_mask) and torch.equal(filled.view(torch.int64), want_filled.view(torch.int64))
    assert torch.equal(work.view(torch.int64), want_filled.view(torch.int64))
    assert torch.equal(out["bin_index"], ref_out["bin_index"]) and info.sf == ref_info.sf
    assert bool((dec[holes] == fill).all())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lo = {k: float(np.min(v)) for k, v in ms.items()}
    hi = {k: float(np.max(v)) for k, v in ms.items()}
    gb = {"mask_build, out of place": (16 * n + n / 8) / 1e9, "mask_build, in place": (16 * n + n / 8) / 1e9,
          "mask_build, mask only": (8 * n + n / 8) / 1e9, "device-to-device copy": 16 * n / 1e9,
          "mask_apply, whole array": (n / 8 + 8 * want_count) / 1e9}
    lines = [f"missing-value layer, fp64 {e}^3 EC eb = {eb}, {want_count} of {n} elements 1e36 in smooth blobs ({frac:.3f})",
             f"sf: plain compress {plain.sf:g}, masked {ref_info.sf:g}; exact coefficients: plain {plain.cnt}, masked {ref_cnt}; "
             f"the mask is {8 * words} bytes = {8 * words / n:.3f} bytes per element",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds",
             f"{'call':<28}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}{'TB/s':>8}"]
    for name, _, _ in calls:
        g_ = gb.get(name)
        lines.append(f"{name:<28}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}" +
                     (f"{g_:>10.3f}{g_ / med[name]:>8.2f}" if g_ else f"{'':>10}{'':>8}"))
    sep = med["compress_masked"] - med["compress(filled)"]
    lines.append(f"compress_masked - compress(filled) = {sep:.4f} ms: what a fill fused into k_compress could save at most; "
                 f"mask_build out of place / copy = {med['mask_build, out of place'] / med['device-to-device copy']:.2f}")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stderr.write(text)
    print(json.dumps({"what": "mask_layer", "n": n, "missing": want_count, "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "separate_pass_ms": round(sep, 4)}))
    ctx.close()


if __name__ == "__main__":
    main()
