#!/usr/bin/env python3
"""Tile summaries, measured: one process, the synthetic fp64 512^3 shard (C4's shard 0), EC, eb 1e-3.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported:

  (a) dctzhip_tile_summary without an original   against   dctzhip_decompress
  (b) dctzhip_tile_summary with the original     against   dctzhip_decompress + dctzhip_psnr_terms
both baselines without the decode memo (DCTZHIP_DEC_MEMO=0).

Condition: each new call's median is below the median of what it replaces by more than that baseline's own max - min over
the rounds.  The byte counts (n elements, p the share of coefficients stored exactly): the pair of (b) moves
n (1.06 + 4 p + 8) + 16 n bytes, the summary n (1.06 + 4 p) + 8 n -- 2.7 x at p = 0.05 -- and (a) reads 0.17 GB where the
decode moves 1.24 GB, but is bound by the decode arithmetic.  One JSON line goes to stdout; --out writes the table as text
(profiles/tile_summary.txt).  For kernel times run the same command under
`rocprofv3 --kernel-trace --stats -- python tools/summary_bench.py`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["DCTZHIP_DEC_MEMO"] = "0"                # before the context reads it


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
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("summary_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e, tdt, eb = a.n, torch.float64, 1e-3
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    n = x.numel()
    out, info = ctx.compress(x, eb, dctz_amd.EC)
    idx, tot = ctx.ac_index(out, n)
    assert tot == info.cnt
    p = info.cnt / n
    full = torch.empty(n, dtype=tdt, device=ctx.device)
    res = {}

    def decode():
        ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def decode_psnr():
        decode()
        res["psnr_terms"] = ctx.psnr_terms(x, full)

    def summary():
        res["summary"] = ctx.tile_summary(out, info.cnt, n, tdt, eb, info.sf, index=idx)

    def summary_ref():
        res["summary_ref"] = ctx.tile_summary(out, info.cnt, n, tdt, eb, info.sf, index=idx, ref=x)

    calls = [("decompress", decode), ("tile_summary", summary), ("decompress + psnr_terms", decode_psnr), ("tile_summary, ref", summary_ref)]
    pairs = [("tile_summary", "decompress", "(a)"), ("tile_summary, ref", "decompress + psnr_terms", "(b)")]
    kernels = {}
    ms = {name: [] for name, _ in calls}
    for r in range(a.warmup + a.rounds):
        for name, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
            kernels[name] = ctx.last_kernel(1)
    # the two ways agree on what they measure
    t = res["summary_ref"][1]
    pt = res["psnr_terms"]
    assert (t.xmin, t.xmax, t.emax) == (pt[0], pt[1], pt[2]) and abs(t.esq - pt[3]) <= 1e-9 * pt[3], (t.xmin, t.xmax, t.emax, t.esq, pt)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lo = {k: float(np.min(v)) for k, v in ms.items()}
    hi = {k: float(np.max(v)) for k, v in ms.items()}
    gb = {"decompress": n * (1.0 + 4.0 / 64 + 4 * p + 8) / 1e9, "tile_summary": n * (1.0 + 4.0 / 64 + 4 * p) / 1e9,
          "decompress + psnr_terms": n * (1.0 + 4.0 / 64 + 4 * p + 8 + 16) / 1e9, "tile_summary, ref": n * (1.0 + 4.0 / 64 + 4 * p + 8) / 1e9}
    lines = [f"tile summaries, fp64 {e}^3 EC eb = {eb}, {info.cnt} exact coefficients (p = {p:.4f}), PSNR {t.psnr(n):.3f} dB",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<26}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}  kernel"]
    for name, _ in calls:
        lines.append(f"{name:<26}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}{gb[name]:>10.3f}  {kernels[name]}")
    ok = {}
    for new, old, tag in pairs:
        spread = hi[old] - lo[old]
        ok[tag] = med[new] < med[old] - spread
        lines.append(f"{tag} {old} / {new} = {med[old] / med[new]:.2f} x measured, {gb[old] / gb[new]:.2f} x by the byte counts; "
                     f"baseline max - min = {spread:.4f} ms; condition (median below the baseline's by more than that): "
                     + ("met" if ok[tag] else "NOT met"))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stderr.write(text)
    print(json.dumps({"what": "tile_summary", "n": n, "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "ratio": {tag: round(med[old] / med[new], 3) for new, old, tag in pairs}, "condition_met": ok}))
    ctx.close()


if __name__ == "__main__":
    main()
