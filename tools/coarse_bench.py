#!/usr/bin/env python3
"""Coarse decode, measured: one process, the synthetic fp64 512^3 shard, EC, eb 1e-3.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported:

  dctzhip_decompress                 the full decode of the flat streams, without the decode memo (DCTZHIP_DEC_MEMO=0)
  dctzhip_decompress_coarse          the same streams at factor 2, 4, 8, 16, 32, 64
  dctzhip_decompress_nd              the full decode of the shard compressed in 4 x 4 x 4 tiles
  dctzhip_decompress_coarse_nd       those streams at factor 2, 4

Condition: every coarse call is faster than the full decode it replaces, in the same run.  One JSON line goes to stdout; --out
writes the table as text (profiles/coarse_decode.txt).  For kernel times run the same command under
`rocprofv3 --kernel-trace --stats -- python tools/coarse_bench.py`."""
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
        raise SystemExit("coarse_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e, tdt, eb = a.n, torch.float64, 1e-3
    dims = (e, e, e)
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device)
    n = x.numel()
    out, info = ctx.compress(x.reshape(-1), eb, dctz_amd.EC)
    idx, tot = ctx.ac_index(out, n)
    assert tot == info.cnt
    nout, ninfo = ctx.compress_nd(x.reshape(dims), eb, dctz_amd.EC)
    nidx, ntot = ctx.ac_index(nout, 64 * ctx.nd_blocks(dims))
    assert ntot == ninfo.cnt
    del x
    full = torch.empty(n, dtype=tdt, device=ctx.device)
    calls = [("decompress", "flat", lambda: ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, dctz_amd.EC, dst=full))]
    keep = []
    for f in (2, 4, 8, 16, 32, 64):
        d = torch.empty(-(-n // f), dtype=tdt, device=ctx.device)
        keep.append(d)
        calls.append((f"coarse f={f}", "flat",
                      lambda f=f, d=d: ctx.decompress_coarse(out, info.cnt, n, tdt, eb, info.sf, f, index=idx, mode=dctz_amd.EC, dst=d)))
    calls.append(("decompress_nd", "tiled", lambda: ctx.decompress_nd(nout, ninfo.cnt, dims, tdt, eb, ninfo.sf, dctz_amd.EC, dst=full.view(dims))))
    for f in (2, 4):
        d = torch.empty([-(-v // f) for v in dims], dtype=tdt, device=ctx.device)
        keep.append(d)
        calls.append((f"coarse_nd f={f}", "tiled",
                      lambda f=f, d=d: ctx.decompress_coarse_nd(nout, ninfo.cnt, dims, tdt, eb, ninfo.sf, f, index=nidx, mode=dctz_amd.EC, dst=d)))
    kernels = {}
    ms = {name: [] for name, _, _ in calls}
    for r in range(a.warmup + a.rounds):
        for name, _, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
            kernels[name] = ctx.last_kernel(1)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lo = {k: float(np.min(v)) for k, v in ms.items()}
    base = {"flat": med["decompress"], "tiled": med["decompress_nd"]}
    lines = [f"coarse decode, fp64 {e}^3 EC eb = {eb}, exact coefficients: flat {info.cnt}, tiled {ninfo.cnt}",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<18}{'median ms':>11}{'min ms':>9}{'full / call':>13}  kernel"]
    ok = True
    for name, kind, _ in calls:
        ratio = base[kind] / med[name]
        is_full = name.startswith("decompress")
        if not is_full and not med[name] < base[kind]:
            ok = False
        lines.append(f"{name:<18}{med[name]:>11.4f}{lo[name]:>9.4f}{ratio:>13.2f}  {kernels[name]}" + ("" if is_full or med[name] < base[kind] else "   NOT FASTER"))
    lines.append("condition (every coarse call faster than the full decode it replaces): " + ("met" if ok else "NOT met"))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stderr.write(text)
    print(json.dumps({"what": "coarse", "n": n, "median_ms": {k: round(v, 4) for k, v in med.items()}, "condition_met": ok}))
    ctx.close()


if __name__ == "__main__":
    main()
