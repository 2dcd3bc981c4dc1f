#!/usr/bin/env python3
"""The tile summaries of a tiled array, measured: one process, the bytes of tools/ndfix_bench.py's table
(the synthetic fp64 512^3 shard, C4's shard 0), EC, eb 1e-3, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles, and
  a 8192 x 16384 field in 8 x 8 tiles.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported with min and max:

  dctzhip_decompress_nd                        (a)'s baseline: the reconstruction written to a second array
  dctzhip_tile_summary_nd without d_ref        (a): records and total of the reconstruction, nothing written but the records
  dctzhip_decompress_nd + dctzhip_psnr_terms   (b)'s baseline: what a user runs today for the PSNR; one number, no map
  dctzhip_tile_summary_nd with d_ref           (b): the same terms per stream tile and joined
the baselines without the decode memo (DCTZHIP_DEC_MEMO=0), the new calls through the C ABI on buffers allocated once.

Condition, for each pair: the new call's median is below the baseline's median by more than the baseline's own max - min over
the rounds.  One JSON line per workload goes to stdout; --out writes the tables as text (profiles/tile_summary_nd.txt)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["DCTZHIP_DEC_MEMO"] = "0"                # before the context reads it


def measure(ctx, x, shape, a):
    import numpy as np
    import torch
    import dctz_amd
    from dctz_amd import hip as H
    tdt, eb = torch.float64, 1e-3
    x = x.view(shape)
    n = x.numel()
    npos = 64 * ctx.nd_blocks(shape)
    out, info = ctx.compress_nd(x, eb, dctz_amd.EC)
    idx, tot = ctx.ac_index(out, npos)
    assert tot == info.cnt
    p = info.cnt / npos
    full = torch.empty(shape, dtype=tdt, device=ctx.device)
    tiles = int(ctx.lib.dctzhip_summary_tiles(npos))
    recs = torch.zeros((tiles, 8), dtype=torch.float64, device=ctx.device)
    total = H.TileSummary()
    dims = (C.c_size_t * len(shape))(*shape)
    res = {}

    def summary(ref):
        rc = ctx.lib.dctzhip_tile_summary_nd(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(info.cnt),
                                             idx.data_ptr(), None, len(shape), dims, H.F64, eb, float(info.sf), dctz_amd.EC, ref,
                                             recs.data_ptr(), C.byref(total))
        assert rc == H.OK, rc

    def decode():
        ctx.decompress_nd(out, info.cnt, shape, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def decode_psnr():
        decode()
        res["psnr_terms"] = ctx.psnr_terms(x.view(-1), full.view(-1))

    def summary_plain():
        summary(None)
        res["plain"] = bytes(total)

    def summary_ref():
        summary(x.data_ptr())
        res["ref"] = bytes(total)
        res["psnr"] = total.psnr(n)

    calls = [("decompress_nd", decode), ("tile_summary_nd", summary_plain), ("decompress_nd + psnr_terms", decode_psnr),
             ("tile_summary_nd, d_ref", summary_ref)]
    kernels = {}
    ms = {name: [] for name, _ in calls}
    seen = {}
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
        # the same bytes every round
        for k_ in ("plain", "ref"):
            assert seen.setdefault(k_, res[k_]) == res[k_]
    # what was timed is the summary of this decode: the joined terms are psnr_terms' (the sum within the any-order bound)
    pt = res["psnr_terms"]
    tot = H.TileSummary.from_buffer_copy(res["ref"])
    assert (tot.xmin, tot.xmax, tot.emax) == tuple(pt[:3]), (tot.xmin, tot.xmax, tot.emax, pt)
    u = 2.0 ** -53
    assert abs(tot.esq - pt[3]) <= 2 * (n - 1) * u / (1 - (n - 1) * u) * pt[3], (tot.esq, pt[3])
    assert tot.rmin == float(full.min()) and tot.rmax == float(full.max())
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    lo = {k_: float(np.min(v)) for k_, v in ms.items()}
    hi = {k_: float(np.max(v)) for k_, v in ms.items()}
    streams = npos * (1.0 + 4.0 / 64 + 4 * p)
    gb = {"decompress_nd": (streams + 8 * n) / 1e9, "tile_summary_nd": (streams + 64 * tiles) / 1e9,
          "decompress_nd + psnr_terms": (streams + 8 * n + 16 * n) / 1e9, "tile_summary_nd, d_ref": (streams + 8 * n + 64 * tiles) / 1e9}
    sh = " x ".join(map(str, shape))
    lines = [f"tile summaries, fp64 {sh} in {'8 x 8' if len(shape) == 2 else '4 x 4 x 4'} tiles, EC eb = {eb}, sf = {info.sf:g}, {info.cnt} exact "
             f"coefficients (p = {p:.4f}), {tiles} records",
             f"PSNR from the total = {res['psnr']:.6f} dB, max |x - r| = {tot.emax:.6g} = {tot.emax / (eb * info.sf):.3f} eb sf",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<29}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}  kernel"]
    for name, _ in calls:
        lines.append(f"{name:<29}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}{gb[name]:>10.3f}  {kernels[name]}")
    met = {}
    for tag, new, old in (("a", "tile_summary_nd", "decompress_nd"), ("b", "tile_summary_nd, d_ref", "decompress_nd + psnr_terms")):
        spread = hi[old] - lo[old]
        met[tag] = bool(med[new] < med[old] - spread)
        lines.append(f"({tag}) {old} / {new} = {med[old] / med[new]:.2f} x measured; baseline max - min = {spread:.4f} ms; condition (median below "
                     f"the baseline's by more than that): " + ("met" if met[tag] else "NOT met"))
    js = {"what": "tile_summary_nd", "shape": list(shape), "tiles": tiles, "median_ms": {k_: round(v, 4) for k_, v in med.items()},
          "condition_met": met}
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
        raise SystemExit("ndsummary_bench.py needs the GPU: nothing is measured without one")
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
