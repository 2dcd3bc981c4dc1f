#!/usr/bin/env python3
"""Many coarse boxes of a tiled array in one call, measured: one process, the bytes of the other tiled
benches (the synthetic fp64 512^3 shard, C4's shard 0), EC, eb 1e-3, as
  a 512 x 512 x 512 volume in 4 x 4 x 4 tiles, and
  a 8192 x 16384 field in 8 x 8 tiles.

Per configuration ONE dctzhip_decompress_coarse_boxes_nd call against the same boxes as a loop of
dctzhip_decompress_coarse_box_nd calls, in the same rounds: device events around the list call and around the whole loop, and
the wall clock of the same (synchronised) calls.  Every configuration runs once per round, the rounds are repeated; medians
are reported with max - min.  Every output of both is checked against the slice of the whole coarse array in the same run.

  volume  f = 2            the 64 coarse bricks of 32^3 cells at (16 + 64 i, 16 + 64 j, 16 + 64 k): the ndboxes lattice at half resolution
          f = 4 (DC-only)  64 planes of 1 x 128 x 128
  field   f = 2, f = 4     an 8 x 8 lattice of 256 x 256-cell map tiles
          f = 8 (DC-only)  64 windows of 128 x 128

Condition, per configuration: the list's wall-clock median and the list's device median each lie below the loop's by more
than the loop's max - min.  Reported without a condition: a one-item list against the single call for the volume's central
eighth and one z-plane at f = 2 (the evidence for or against routing the single call through a one-item list), and -- with
--dropin -- 8 boxes from the shard's DZIX DZND container through dctz_decompress_coarse_boxes_nd against 8
dctz_decompress_coarse_box_nd calls, wall clock.  One JSON line per workload goes to stdout; --out writes the tables as text
(profiles/coarse_boxes_nd.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs_of(shape):
    """[(factor, label, [(lo, hi)], condition?)] in coarse coordinates."""
    r8 = range(8)
    if len(shape) == 3:
        c2, c4 = [d // 2 for d in shape], [d // 4 for d in shape]
        step = c2[0] // 4
        bricks = [((step // 4 + step * i, step // 4 + step * j, step // 4 + step * k),
                   (step // 4 + step * i + step // 2, step // 4 + step * j + step // 2, step // 4 + step * k + step // 2))
                  for i in range(4) for j in range(4) for k in range(4)]
        planes = [((c4[0] * i // 64, 0, 0), (c4[0] * i // 64 + 1, c4[1], c4[2])) for i in range(64)]
        eighth = (tuple(d // 4 for d in c2), tuple(d // 4 + d // 2 for d in c2))
        zplane = ((c2[0] // 2, 0, 0), (c2[0] // 2 + 1, c2[1], c2[2]))
        return [(2, "64 bricks of 32^3", bricks, True), (4, "64 DC planes 1 x 128 x 128", planes, True),
                (2, "central eighth, one item", [eighth], False), (2, "z-plane, one item", [zplane], False)]
    cfg = []
    for f, edge, label in ((2, 256, "64 map tiles 256 x 256"), (4, 256, "64 map tiles 256 x 256"), (8, 128, "64 DC windows 128 x 128")):
        cd = [d // f for d in shape]
        sy, sx = cd[0] // 8, cd[1] // 8
        assert edge <= sy and edge <= sx
        bx = [(((sy - edge) // 2 + sy * i, (sx - edge) // 2 + sx * j), ((sy - edge) // 2 + sy * i + edge, (sx - edge) // 2 + sx * j + edge))
              for i in r8 for j in r8]
        cfg.append((f, label, bx, True))
    return cfg


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
    cfg = configs_of(shape)
    whole = {f: ctx.decompress_coarse_nd(out, info.cnt, shape, tdt, eb, info.sf, f, index=idx, mode=dctz_amd.EC) for f in sorted({c[0] for c in cfg})}
    runs = []
    for f, label, bx, cond in cfg:
        d_list = [torch.empty([h - l for l, h in zip(lo, hi)], dtype=tdt, device=ctx.device) for lo, hi in bx]
        d_loop = [torch.empty_like(d) for d in d_list]

        def f_list(f=f, bx=bx, d=d_list):
            ctx.decompress_coarse_boxes_nd(out, info.cnt, shape, tdt, eb, info.sf, f, bx, index=idx, mode=dctz_amd.EC, dsts=d)

        def f_loop(f=f, bx=bx, d=d_loop):
            for (lo, hi), o in zip(bx, d):
                ctx.decompress_coarse_box_nd(out, info.cnt, shape, tdt, eb, info.sf, f, lo, hi, index=idx, mode=dctz_amd.EC, dst=o)

        runs.append({"f": f, "label": label, "boxes": bx, "cond": cond, "list": f_list, "loop": f_loop, "d_list": d_list, "d_loop": d_loop,
                     "ms": {"list": ([], []), "loop": ([], [])}})
    for r in range(a.warmup + a.rounds):
        for run in runs:
            for which in ("loop", "list"):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                t0.record()
                run[which]()
                t1.record()
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                if r >= a.warmup:
                    run["ms"][which][0].append(t0.elapsed_time(t1))
                    run["ms"][which][1].append((w1 - w0) * 1e3)
                if which == "list":
                    run["kernel"] = ctx.last_kernel(1)
                    run["ctr"] = (ctx.counter(13), ctx.counter(14), ctx.counter(15))
        if r == 0:                                      # what is timed is the slice of the whole coarse array
            for run in runs:
                for (lo, hi), dl, dp in zip(run["boxes"], run["d_list"], run["d_loop"]):
                    want = whole[run["f"]][tuple(slice(l, h) for l, h in zip(lo, hi))].contiguous()
                    assert torch.equal(dl.view(torch.int64), want.view(torch.int64)), (run["label"], lo, hi)
                    assert torch.equal(dp.view(torch.int64), want.view(torch.int64)), (run["label"], lo, hi)
    sh = " x ".join(map(str, shape))
    lines = [f"many coarse boxes in one call, fp64 {sh} in {'8 x 8' if len(shape) == 2 else '4 x 4 x 4'} tiles, EC eb = {eb}, sf = {info.sf:g}, "
             f"{info.cnt} exact coefficients (p = {info.cnt / npos:.4f}), {npos // 4096} stream tiles",
             f"device events and wall clock around each synchronised call (the loop: around all its calls), {a.rounds} alternating rounds "
             f"after {a.warmup} warm-up rounds; median ms (max - min)",
             f"{'configuration':<36}{'k':>4}{'loop dev':>18}{'list dev':>18}{'loop wall':>18}{'list wall':>18}{'dev x':>8}{'wall x':>8}"
             f"{'items':>7}{'wgs':>7}{'bound':>7}  kernel"]
    js = {"what": "coarse_boxes_nd", "shape": list(shape), "rows": []}
    for run in runs:
        st = {}
        for which in ("loop", "list"):
            for j, clock in enumerate(("dev", "wall")):
                v = run["ms"][which][j]
                st[which, clock] = (float(np.median(v)), float(np.max(v) - np.min(v)))
        cell = lambda k_: f"{st[k_][0]:>10.4f} ({st[k_][1]:.4f})".rjust(18)
        rd, rw = st["loop", "dev"][0] / st["list", "dev"][0], st["loop", "wall"][0] / st["list", "wall"][0]
        name = f"f={run['f']} {run['label']}"
        it, wg, bd = run["ctr"]
        lines.append(f"{name:<36}{len(run['boxes']):>4}{cell(('loop', 'dev'))}{cell(('list', 'dev'))}{cell(('loop', 'wall'))}{cell(('list', 'wall'))}"
                     f"{rd:>8.2f}{rw:>8.2f}{it:>7}{wg:>7}{bd:>7}  {run['kernel']}")
        row = {"config": name, "k": len(run["boxes"]), "loop_dev_ms": round(st["loop", "dev"][0], 4), "list_dev_ms": round(st["list", "dev"][0], 4),
               "loop_wall_ms": round(st["loop", "wall"][0], 4), "list_wall_ms": round(st["list", "wall"][0], 4), "dev_ratio": round(rd, 2),
               "wall_ratio": round(rw, 2)}
        if run["cond"]:
            met = bool(st["list", "dev"][0] < st["loop", "dev"][0] - st["loop", "dev"][1] and
                       st["list", "wall"][0] < st["loop", "wall"][0] - st["loop", "wall"][1])
            row["condition_met"] = met
            lines.append(f"    condition (list medians below the loop's by more than the loop's max - min, device and wall): " + ("met" if met else "NOT met"))
        else:
            lines.append("    reported, no condition: a one-item list against the single call")
        js["rows"].append(row)
    return "\n".join(lines) + "\n", js


def dropin(a, W):
    """8 boxes from the shard's DZIX DZND container, f = 2: one dctz_decompress_coarse_boxes_nd against 8 dctz_decompress_coarse_box_nd."""
    import ctypes as C
    import numpy as np

    class Buf(C.Union):
        _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]

    class TVar(C.Structure):                        # include/dctz.h: t_var
        _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", Buf)]

    def tv(arr):
        v = TVar()
        v.datatype = 1
        v.buf.d = arr.ctypes.data_as(C.POINTER(C.c_double))
        return v

    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(ROOT, "dctz_amd", "lib", "libdctz-ec.so"))
    lib.dctz_compress.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(TVar), C.c_double]
    lib.dctz_set_block_dims.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    lib.dctz_decompress_coarse_box_nd.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(TVar)]
    lib.dctz_decompress_coarse_boxes_nd.argtypes = [C.POINTER(TVar), C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                    C.POINTER(C.POINTER(TVar))]
    e = a.n
    dims = (e, e, e)
    arr = lambda v: (C.c_size_t * len(v))(*v)
    x = W.c3(e, seed=512)
    n = x.size
    z = np.empty(n + (1 << 20), np.float64)
    sz = C.c_size_t(0)
    os.environ["DCTZ_ZLIB_GPU"] = "1"
    assert lib.dctz_set_block_dims(3, arr(dims)) == 0
    assert lib.dctz_compress(C.byref(tv(x)), n, C.byref(sz), C.byref(tv(z)), 1e-3) == 1
    del os.environ["DCTZ_ZLIB_GPU"]
    bx = configs_of(dims)[0][2][21:43:3]            # 8 bricks from the middle of the lattice
    assert len(bx) == 8
    cells = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in bx]
    one = [np.empty(c, np.float64) for c in cells]
    many = [np.empty(c, np.float64) for c in cells]
    tvs = [tv(o) for o in many]
    ptrs = (C.POINTER(TVar) * len(bx))(*[C.pointer(t) for t in tvs])
    los, his = arr([v for lo, hi in bx for v in lo]), arr([v for lo, hi in bx for v in hi])

    def t_loop():
        for (lo, hi), o in zip(bx, one):
            assert lib.dctz_decompress_coarse_box_nd(C.byref(tv(z)), 2, arr(lo), arr(hi), C.byref(tv(o))) == 1

    def t_list():
        assert lib.dctz_decompress_coarse_boxes_nd(C.byref(tv(z)), 2, len(bx), los, his, ptrs) == 1

    ts = {"loop": [], "list": []}
    for r in range(2 + max(3, a.rounds // 4)):
        for name, f in (("loop", t_loop), ("list", t_list)):
            t0 = time.perf_counter()
            f()
            if r >= 2:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    for o, m in zip(one, many):
        assert np.array_equal(o.view(np.uint64), m.view(np.uint64))
    ms_loop, ms_list = float(np.median(ts["loop"])), float(np.median(ts["list"]))
    text = (f"drop-in, the shard's DZIX DZND container ({sz.value} bytes), f = 2, 8 bricks of {cells[0]} cells, wall clock, median of "
            f"{len(ts['loop'])} rounds:\n  8 x dctz_decompress_coarse_box_nd {ms_loop:.3f} ms (max - min {max(ts['loop']) - min(ts['loop']):.3f}); "
            f"dctz_decompress_coarse_boxes_nd {ms_list:.3f} ms (max - min {max(ts['list']) - min(ts['list']):.3f}); ratio {ms_loop / ms_list:.2f}\n")
    js = {"what": "coarse_boxes_nd", "via": "dropin", "n": n, "container_bytes": sz.value, "boxes": len(bx),
          "wall_ms_8x_dctz_decompress_coarse_box_nd": round(ms_loop, 3), "wall_ms_dctz_decompress_coarse_boxes_nd": round(ms_list, 3)}
    return text, js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="edge of the cube; the 2-D workload is the same bytes as n^2 / 32 x 32 n")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropin", action="store_true", help="also 8 boxes through the drop-in library, from a DZIX DZND container")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dctz_amd
    from tests import workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("coarse_boxes_bench.py needs the GPU: nothing is measured without one")
    ctx = dctz_amd.Context(0)
    e = a.n
    x = torch.from_numpy(W.c3(e, seed=512)).to(ctx.device).reshape(-1)
    text = ""
    for shape in ((e, e, e), (e * e // 32, 32 * e)):
        t, js = measure(ctx, x, shape, a)
        text += t + "\n"
        sys.stderr.write(t + "\n")
        print(json.dumps(js), flush=True)
    ctx.close()
    del x
    if a.dropin:
        t, js = dropin(a, W)
        text += t + "\n"
        sys.stderr.write(t + "\n")
        print(json.dumps(js), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
