#!/usr/bin/env python3
"""A box of the coarse decode of a tiled array, measured: one process, the bytes of the other tiled
benches (the synthetic fp64 512^3 shard, C4's shard 0), EC, eb 1e-3, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles, and
  a 8192 x 16384 field in 8 x 8 tiles.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported with min and max:

  dctzhip_decompress_coarse_nd       the baseline: the whole array at factor f -- the only way to these values without the box call
  dctzhip_decompress_coarse_box_nd   volume, f = 2: one coarse z-plane (1 x 256 x 256) and the central eighth (128^3);
                                     volume, f = 4: one plane of the DC grid (1 x 128 x 128);
                                     field, f = 2, 4, 8: a centred window of a quarter of each coarse extent

Every box is checked once against the slice of the whole-array call, bit for bit.  Condition, for each box: its median is
below its baseline's median by more than the baseline's own max - min over the rounds.  One JSON line per workload goes to
stdout; --out writes the tables as text (profiles/coarse_box_nd.txt)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes_of(shape):
    """[(factor, label, lo, hi)] in coarse coordinates."""
    if len(shape) == 3:
        c2, c4 = [d // 2 for d in shape], [d // 4 for d in shape]
        return [(2, "z-plane", (c2[0] // 2, 0, 0), (c2[0] // 2 + 1, c2[1], c2[2])),
                (2, "central eighth", tuple(d // 4 for d in c2), tuple(d // 4 + d // 2 for d in c2)),
                (4, "DC plane", (c4[0] // 2, 0, 0), (c4[0] // 2 + 1, c4[1], c4[2]))]
    bx = []
    for f in (2, 4, 8):
        cd = [d // f for d in shape]
        bx.append((f, "centred quarter window", tuple(d * 3 // 8 for d in cd), tuple(d * 3 // 8 + d // 4 for d in cd)))
    return bx


def measure(ctx, x, shape, a):
    import numpy as np
    import torch
    import dctz_amd
    tdt, eb = torch.float64, 1e-3
    x = x.view(shape)
    npos = 64 * ctx.nd_blocks(shape)
    out, info = ctx.compress_nd(x, eb, dctz_amd.EC)
    idx, tot = ctx.ac_index(out, npos)
    assert tot == info.cnt
    bx = boxes_of(shape)
    whole = {f: torch.empty([-(-d // f) for d in shape], dtype=tdt, device=ctx.device) for f in sorted({b[0] for b in bx})}
    calls = []
    for f, w in whole.items():
        calls.append((f"coarse_nd f={f}", None, f,
                      lambda f=f, w=w: ctx.decompress_coarse_nd(out, info.cnt, shape, tdt, eb, info.sf, f, index=idx, mode=dctz_amd.EC, dst=w)))
    for f, label, lo, hi in bx:
        d = torch.empty([h - l for l, h in zip(lo, hi)], dtype=tdt, device=ctx.device)
        calls.append((f"box f={f} {label}", (lo, hi, d), f,
                      lambda f=f, lo=lo, hi=hi, d=d: ctx.decompress_coarse_box_nd(out, info.cnt, shape, tdt, eb, info.sf, f, lo, hi, index=idx,
                                                                                  mode=dctz_amd.EC, dst=d)))
    kernels, grids = {}, {}
    ms = {name: [] for name, _, _, _ in calls}
    for r in range(a.warmup + a.rounds):
        for name, box, f, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
            kernels[name] = ctx.last_kernel(1)
            if box is not None:
                grids[name] = (ctx.counter(11), ctx.counter(12))
        if r == 0:                                      # what is timed is the slice of the baseline
            for name, box, f, _ in calls:
                if box is not None:
                    lo, hi, d = box
                    want = whole[f][tuple(slice(l, h) for l, h in zip(lo, hi))].contiguous()
                    assert torch.equal(d.view(torch.int64), want.view(torch.int64)), name
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    lo_ = {k_: float(np.min(v)) for k_, v in ms.items()}
    hi_ = {k_: float(np.max(v)) for k_, v in ms.items()}
    sh = " x ".join(map(str, shape))
    lines = [f"coarse box decode, fp64 {sh} in {'8 x 8' if len(shape) == 2 else '4 x 4 x 4'} tiles, EC eb = {eb}, sf = {info.sf:g}, {info.cnt} exact "
             f"coefficients (p = {info.cnt / npos:.4f}), {npos // 4096} stream tiles",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds",
             f"{'call':<34}{'box (coarse cells)':<22}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'wgs':>7}{'cand.':>7}  kernel"]
    met = {}
    for name, box, f, _ in calls:
        ext = "whole" if box is None else " x ".join(str(h - l) for l, h in zip(box[0], box[1]))
        g, t = grids.get(name, ("", ""))
        lines.append(f"{name:<34}{ext:<22}{med[name]:>11.4f}{lo_[name]:>9.4f}{hi_[name]:>9.4f}{g:>7}{t:>7}  {kernels[name]}")
    for name, box, f, _ in calls:
        if box is None:
            continue
        old = f"coarse_nd f={f}"
        spread = hi_[old] - lo_[old]
        met[name] = bool(med[name] < med[old] - spread)
        lines.append(f"{name}: {old} / box = {med[old] / med[name]:.2f} x measured; baseline max - min = {spread:.4f} ms; condition (median below "
                     f"the baseline's by more than that): " + ("met" if met[name] else "NOT met"))
    js = {"what": "coarse_box_nd", "shape": list(shape), "median_ms": {k_: round(v, 4) for k_, v in med.items()}, "condition_met": met}
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
        raise SystemExit("coarse_box_bench.py needs the GPU: nothing is measured without one")
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
