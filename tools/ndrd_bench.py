#!/usr/bin/env python3
"""The rate-distortion probe of a tiled array, measured: one process, the bytes of the synthetic fp64 512^3
shard (C4's shard 0), EC, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles and a 8192 x 16384 field in 8 x 8 tiles (no padding), and
  their ragged twins 511 x 509 x 510 and 8191 x 16381 (the first elements of the same buffer; every axis padded).

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported with min and max:

  dctzhip_rd_probe_nd, K = 7, 9, 16                              the new call (7 and 9: the two probes of compress_psnr_nd)
  16 x (compress_nd + decompress_nd + psnr_terms)                what it replaces: the reference's sweep, one bound after the other
  dctzhip_rd_probe, K = 16                                       the flat probe over the same buffer, for comparison only
  dctzhip_compress_psnr_nd at 60 and 80 dB                       end to end: two probes, compress, decode, measure
the sweep without the decode memo (DCTZHIP_DEC_MEMO=0).

Condition, per workload: the K = 16 probe's median is below the sweep's median by more than the sweep's own max - min over the
rounds.  One JSON line per workload goes to stdout; --out writes the tables as text (profiles/rd_probe_nd.txt)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["DCTZHIP_DEC_MEMO"] = "0"                # before the context reads it

EBS = [1e-6, 2e-6, 5e-6, 1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0]


def measure(ctx, buf, shape, a):
    import numpy as np
    import torch
    import dctz_amd
    from dctz_amd import hip as H
    tdt = torch.float64
    n = int(np.prod(shape))
    x = buf[:n].view(shape)
    flat = buf[:n]
    out = ctx.alloc_outputs(64 * ctx.nd_blocks(shape), tdt)
    full = torch.empty(shape, dtype=tdt, device=ctx.device)
    grid = H.psnr_grid()
    res = {}

    def probe(k):
        def fn():
            res[f"probe{k}"] = ctx.rd_probe_nd(x, (EBS if k == 16 else grid[0:61:10] if k == 7 else grid[31:40])[:k])
        return fn

    def sweep():
        got = []
        for eb in EBS:
            _, info = ctx.compress_nd(x, eb, dctz_amd.EC, out=out)
            ctx.decompress_nd(out, info.cnt, shape, tdt, eb, info.sf, dctz_amd.EC, dst=full)
            got.append((info.cnt, ctx.psnr_terms(flat, full.view(-1))))
        res["sweep"] = got

    def flat_probe():
        res["flat"] = ctx.rd_probe(flat, EBS)

    def target(db):
        def fn():
            _, _, eb, ps = ctx.compress_psnr_nd(x, db, out=out)
            res[f"psnr{db}"] = (eb, ps)
        return fn

    calls = [("rd_probe_nd K=7", probe(7)), ("rd_probe_nd K=9", probe(9)), ("rd_probe_nd K=16", probe(16)),
             ("16 x (compress_nd + decompress_nd + psnr_terms)", sweep), ("rd_probe (flat blocks) K=16", flat_probe),
             ("compress_psnr_nd 60 dB", target(60)), ("compress_psnr_nd 80 dB", target(80))]
    ms = {name: [] for name, _ in calls}
    seen = None
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
        # the same results every round
        seen = seen or res["probe16"]
        assert seen == res["probe16"]
    # what was timed answers the sweep's question: the counts exactly, the SSE to the probe's rule
    pts, rng = res["probe16"]
    worst = 0.0
    for p, (cnt, t) in zip(pts, res["sweep"]):
        assert p["cnt"] == cnt and rng == (t[0], t[1]), (p, cnt, t)
        assert abs(p["sse"] - t[3]) <= 1e-8 * t[3], (p, t)
        worst = max(worst, abs(p["sse"] - t[3]) / t[3])
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    lo = {k_: float(np.min(v)) for k_, v in ms.items()}
    hi = {k_: float(np.max(v)) for k_, v in ms.items()}
    sh = " x ".join(map(str, shape))
    lines = [f"rate-distortion probe, fp64 {sh} in {'8 x 8' if len(shape) == 2 else '4 x 4 x 4'} tiles, EC, {ctx.nd_blocks(shape)} tiles, "
             f"{n * 8 / 2 ** 30:.3f} GiB",
             f"worst relative miss of the predicted SSE against the sweep's measured one over the 16 bounds: {worst:.2e}",
             f"compress_psnr_nd: 60 dB -> eb {res['psnr60'][0]:g} ({res['psnr60'][1]:.3f} dB), 80 dB -> eb {res['psnr80'][0]:g} ({res['psnr80'][1]:.3f} dB)",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<50}{'median ms':>11}{'min ms':>9}{'max ms':>9}"]
    for name, _ in calls:
        lines.append(f"{name:<50}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}")
    new, old, fl = "rd_probe_nd K=16", "16 x (compress_nd + decompress_nd + psnr_terms)", "rd_probe (flat blocks) K=16"
    spread = hi[old] - lo[old]
    met = bool(med[new] < med[old] - spread)
    lines.append(f"sweep / probe (K = 16) = {med[old] / med[new]:.2f} x measured; the sweep's max - min = {spread:.4f} ms; condition (median below "
                 f"the sweep's by more than that): " + ("met" if met else "NOT met"))
    lines.append(f"tiled probe / flat probe (K = 16) = {med[new] / med[fl]:.3f}")
    js = {"what": "rd_probe_nd", "shape": list(shape), "median_ms": {k_: round(v, 4) for k_, v in med.items()}, "condition_met": met}
    return "\n".join(lines) + "\n", js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="edge of the cube; the 2-D workload is the same bytes as n^2 / 32 x 32 n")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dctz_amd
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("ndrd_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e = a.n
    buf = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    text = ""
    results = []
    for shape in ((e, e, e), (e - 1, e - 3, e - 2), (e * e // 32, 32 * e), (e * e // 32 - 1, 32 * e - 3)):
        t, js = measure(ctx, buf, shape, a)
        results.append(js)
        text += t + "\n"
        sys.stderr.write(t + "\n")
        print(json.dumps(js), flush=True)
    # what the edge pass costs: the ragged twin against the aligned workload, per element
    k = "rd_probe_nd K=16"
    for al, rg in ((0, 1), (2, 3)):
        na, nr = 1, 1
        for d in results[al]["shape"]:
            na *= d
        for d in results[rg]["shape"]:
            nr *= d
        ta, tr = results[al]["median_ms"][k], results[rg]["median_ms"][k]
        line = (f"ragged {' x '.join(map(str, results[rg]['shape']))} against {' x '.join(map(str, results[al]['shape']))}, K = 16: "
                f"{tr:.4f} ms against {ta:.4f} ms = {100 * (tr / ta - 1):+.1f} % ({100 * (tr / nr / (ta / na) - 1):+.1f} % per element)\n")
        text += line
        sys.stderr.write(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
