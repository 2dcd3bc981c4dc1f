#!/usr/bin/env python3
"""The correction list of a tiled array, measured: one process, the bytes of tools/fixup_bench.py's
table (the synthetic fp64 512^3 shard, C4's shard 0), EC, eb 1e-3, bound = eb sf, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles, and
  a 8192 x 16384 field in 8 x 8 tiles.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported with min and max:

  dctzhip_decompress_nd + dctzhip_psnr_terms   what a user runs today: reads the same data, yields one number (max |x - r|)
  dctzhip_fixup_build_nd, count only           "what would this bound cost?"
  dctzhip_fixup_build_nd with the list         into buffers of exactly the counted capacity
  dctzhip_fixup_apply_nd                       the whole array, on the decode the pair left behind
the baseline without the decode memo (DCTZHIP_DEC_MEMO=0), the new calls through the C ABI on buffers allocated once.

Condition: the median of the build with the list is below the pair's median by more than the pair's own max - min over the
rounds.  Apply has no condition.  One JSON line per workload goes to stdout; --out writes the tables as text
(profiles/ndfix_list.txt)."""
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
    bound = a.mult * eb * info.sf
    full = torch.empty(shape, dtype=tdt, device=ctx.device)
    # the list once through the binding: its size, and the buffers the timed calls write
    start, off, val, k = ctx.fixup_build_nd(out, info.cnt, shape, tdt, eb, info.sf, x, bound, index=idx)
    want = (start.clone(), off.clone(), val.clone())
    count = C.c_uint32(0)
    dims = (C.c_size_t * len(shape))(*shape)
    res = {}

    def build(o, v, cap):
        rc = ctx.lib.dctzhip_fixup_build_nd(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(info.cnt),
                                            idx.data_ptr(), None, len(shape), dims, H.F64, eb, float(info.sf), dctz_amd.EC, x.data_ptr(), bound,
                                            start.data_ptr(), o, v, cap, C.byref(count))
        assert rc == H.OK and count.value == k, (rc, count.value, k)

    def decode_psnr():
        ctx.decompress_nd(out, info.cnt, shape, tdt, eb, info.sf, dctz_amd.EC, dst=full)
        res["psnr_terms"] = ctx.psnr_terms(x.view(-1), full.view(-1))

    def count_only():
        build(None, None, 0)

    def with_list():
        build(off.data_ptr(), val.data_ptr(), k)

    def apply():
        ctx.fixup_apply_nd((start, off, val, k), shape, tdt, full)

    calls = [("decompress_nd + psnr_terms", decode_psnr), ("fixup_build_nd, count only", count_only), ("fixup_build_nd, list", with_list),
             ("fixup_apply_nd, whole array", apply)]
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
    # what was timed is the list, and the applied decode keeps the bound
    assert all(torch.equal(g, w) for g, w in zip((start, off, val), want))
    emax = res["psnr_terms"][2]
    within = ((x - full).abs() <= bound) | (x == full)
    assert bool(within.all())
    after = float((x - full).abs().max())
    del within
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    lo = {k_: float(np.min(v)) for k_, v in ms.items()}
    hi = {k_: float(np.max(v)) for k_, v in ms.items()}
    tiles = int(ctx.lib.dctzhip_fixup_tiles(npos))
    list_bytes = 4 * (tiles + 1) + k * (2 + 8)
    streams = npos * (1.0 + 4.0 / 64 + 4 * p)
    gb = {"decompress_nd + psnr_terms": (streams + 8 * n + 16 * n) / 1e9, "fixup_build_nd, count only": (streams + 8 * n + npos / 8) / 1e9,
          "fixup_build_nd, list": (streams + 8 * n + 2 * npos / 8 + 4 * tiles + k * 18) / 1e9,
          "fixup_apply_nd, whole array": (4 * tiles + k * 18) / 1e9}
    sh = " x ".join(map(str, shape))
    lines = [f"correction list, fp64 {sh} in {'8 x 8' if len(shape) == 2 else '4 x 4 x 4'} tiles, EC eb = {eb}, sf = {info.sf:g}, {info.cnt} exact "
             f"coefficients (p = {p:.4f}), bound = {a.mult:g} eb sf = {bound:g}",
             f"max |x - r| = {emax:.6g} = {emax / (eb * info.sf):.3f} eb sf before, {after:.6g} after apply; {k} of {n} elements listed "
             f"({k / n:.3e}), the list is {list_bytes} bytes = {list_bytes / n:.3e} bytes per element",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<29}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}  kernel"]
    for name, _ in calls:
        lines.append(f"{name:<29}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}{gb[name]:>10.3f}  {kernels[name]}")
    new, old = "fixup_build_nd, list", "decompress_nd + psnr_terms"
    spread = hi[old] - lo[old]
    ok = med[new] < med[old] - spread
    lines.append(f"{old} / {new} = {med[old] / med[new]:.2f} x measured; baseline max - min = {spread:.4f} ms; condition (median below the "
                 f"baseline's by more than that): " + ("met" if ok else "NOT met"))
    js = {"what": "ndfix_list", "shape": list(shape), "listed": k, "list_bytes_per_element": list_bytes / n,
          "median_ms": {k_: round(v, 4) for k_, v in med.items()}, "ratio": round(med[old] / med[new], 3), "condition_met": bool(ok)}
    return "\n".join(lines) + "\n", js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="edge of the cube; the 2-D workload is the same bytes as n^2 / 32 x 32 n")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mult", type=float, default=1.0, help="the bound in units of eb sf")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dctz_amd
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("ndfix_bench.py needs the GPU: nothing is measured without one")
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
