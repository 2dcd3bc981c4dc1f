#!/usr/bin/env python3
"""The correction list for a point-wise bound, measured: one process, the synthetic fp64 512^3 shard
(C4's shard 0), EC, eb 1e-3, bound = eb sf.

Timed with device events around each call, every call of a round once, the rounds repeated (so that the calls alternate and
share whatever else the machine is doing); the median over the rounds is reported:

  dctzhip_decompress + dctzhip_psnr_terms   the existing pair that reads the same data and yields one number (max |x - r|)
  dctzhip_fixup_build, count only           "what would this bound cost?"
  dctzhip_fixup_build with the list         into buffers of exactly the counted capacity
  dctzhip_fixup_apply                       the whole array, on the decode the pair left behind
the baseline without the decode memo (DCTZHIP_DEC_MEMO=0), the new calls through the C ABI on buffers allocated once.

Condition: the median of the build with the list is below the pair's median by more than the pair's own max - min over the
rounds.  Apply has no condition.  One JSON line goes to stdout; --out writes the table as text (profiles/fixup_list.txt).
For kernel times run the same command under `rocprofv3 --kernel-trace --stats -- python tools/fixup_bench.py`."""
import argparse
import ctypes as C
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
    ap.add_argument("--mult", type=float, default=1.0, help="the bound in units of eb sf")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dctz_amd
    from dctz_amd import hip as H
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("fixup_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e, tdt, eb = a.n, torch.float64, 1e-3
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    n = x.numel()
    out, info = ctx.compress(x, eb, dctz_amd.EC)
    idx, tot = ctx.ac_index(out, n)
    assert tot == info.cnt
    p = info.cnt / n
    bound = a.mult * eb * info.sf
    full = torch.empty(n, dtype=tdt, device=ctx.device)
    # the list once through the binding: its size, and the buffers the timed calls write
    start, off, val, k = ctx.fixup_build(out, info.cnt, n, tdt, eb, info.sf, x, bound, index=idx)
    want = (start.clone(), off.clone(), val.clone())
    count = C.c_uint32(0)
    res = {}

    def build(o, v, cap):
        rc = ctx.lib.dctzhip_fixup_build(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(info.cnt),
                                         idx.data_ptr(), None, n, H.F64, eb, float(info.sf), dctz_amd.EC, x.data_ptr(), bound, start.data_ptr(),
                                         o, v, cap, C.byref(count))
        assert rc == H.OK and count.value == k, (rc, count.value, k)

    def decode_psnr():
        ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, dctz_amd.EC, dst=full)
        res["psnr_terms"] = ctx.psnr_terms(x, full)

    def count_only():
        build(None, None, 0)

    def with_list():
        build(off.data_ptr(), val.data_ptr(), k)

    def apply():
        ctx.fixup_apply((start, off, val, k), n, tdt, full)

    calls = [("decompress + psnr_terms", decode_psnr), ("fixup_build, count only", count_only), ("fixup_build, list", with_list),
             ("fixup_apply, whole array", apply)]
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
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    lo = {k_: float(np.min(v)) for k_, v in ms.items()}
    hi = {k_: float(np.max(v)) for k_, v in ms.items()}
    tiles = int(ctx.lib.dctzhip_fixup_tiles(n))
    list_bytes = 4 * (tiles + 1) + k * (2 + 8)
    streams = n * (1.0 + 4.0 / 64 + 4 * p)
    gb = {"decompress + psnr_terms": (streams + 8 * n + 16 * n) / 1e9, "fixup_build, count only": (streams + 8 * n + n / 8) / 1e9,
          "fixup_build, list": (streams + 8 * n + 2 * n / 8 + 4 * tiles + k * 18) / 1e9, "fixup_apply, whole array": (4 * tiles + k * 18) / 1e9}
    lines = [f"correction list, fp64 {e}^3 EC eb = {eb}, sf = {info.sf:g}, {info.cnt} exact coefficients (p = {p:.4f}), bound = {a.mult:g} eb sf = {bound:g}",
             f"max |x - r| = {emax:.6g} = {emax / (eb * info.sf):.3f} eb sf before, {after:.6g} after apply; {k} of {n} elements listed "
             f"({k / n:.3e}), the list is {list_bytes} bytes = {list_bytes / n:.3e} bytes per element",
             f"device events around each call, {a.rounds} alternating rounds after {a.warmup} warm-up rounds, DCTZHIP_DEC_MEMO=0",
             f"{'call':<26}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'GB moved':>10}  kernel"]
    for name, _ in calls:
        lines.append(f"{name:<26}{med[name]:>11.4f}{lo[name]:>9.4f}{hi[name]:>9.4f}{gb[name]:>10.3f}  {kernels[name]}")
    new, old = "fixup_build, list", "decompress + psnr_terms"
    spread = hi[old] - lo[old]
    ok = med[new] < med[old] - spread
    lines.append(f"{old} / {new} = {med[old] / med[new]:.2f} x measured; baseline max - min = {spread:.4f} ms; condition (median below the "
                 f"baseline's by more than that): " + ("met" if ok else "NOT met"))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stderr.write(text)
    print(json.dumps({"what": "fixup_list", "n": n, "listed": k, "list_bytes_per_element": list_bytes / n,
                      "median_ms": {k_: round(v, 4) for k_, v in med.items()}, "ratio": round(med[old] / med[new], 3), "condition_met": bool(ok)}))
    ctx.close()


if __name__ == "__main__":
    main()
