#!/usr/bin/env python3
"""Random access on decode, measured: the exception index and range decodes of the C4 shard
(synthetic fp64 512^3, EC, eb 1e-3) next to the whole-array decode in the same process.

  --what index   dctzhip_ac_index               (k_ac_index*)
  --what range   2^21 contiguous elements       (k_decompress_range)
  --what one     one element                    (wall clock of the call)
  --what full    [0, n)
  --what dropin  dctz_decompress_range of 2^21 elements from the shard's 1 GiB DZIX container (DCTZ_ZLIB_GPU=1)
                 against dctz_decompress of the whole container (wall clock, host buffers)
  --what box     a box of the shard through --via box (dctzhip_decompress_box: k_decompress_box), --via ranges (one
                 dctzhip_decompress_range call per run of the box, into the right offsets) or --via slice (whole decode +
                 torch slice copy); --box brick (64^3 at 224^3) | zplane ([100:101, :, :]) | xplane ([:, :, 100:101]) |
                 full | c2 (the 1800 x 3600 fp32 field, window [600:856, 1200:1712])
  --what ndbox   the same boxes (brick | zplane | xplane | full) of the shard compressed in 4 x 4 x 4 tiles (compress_nd)
                 through dctzhip_decompress_box_nd (k_decompress_ndbox), beside that run's whole-array decompress_nd
  --what boxes   many boxes of the shard in one call: --via list (the 64 disjoint 64^3 bricks at (32 + 128 i, 32 + 128 j,
                 32 + 128 k) through ONE dctzhip_decompress_boxes call: k_boxlist_build + k_decompress_mbox), --via loop
                 (the same bricks as 64 dctzhip_decompress_box calls), --via one (the single brick at 224^3 through the
                 list call), --via dropin (8 of the bricks from the shard's 1 GiB DZIX container: dctz_decompress_boxes
                 against 8 dctz_decompress_box calls, wall clock, host buffers)
  --what ndboxes the same lists for the shard compressed in 4 x 4 x 4 tiles (compress_nd): --via list (the 64 bricks through
                 ONE dctzhip_decompress_boxes_nd call: k_boxlist_build + k_decompress_mbox_nd), --via loop (64
                 dctzhip_decompress_box_nd calls), --via one (--box brick | xplane | zplane | full as a one-item list),
                 --via dropin (8 of the bricks from the shard's DZIX DZND container: dctz_decompress_boxes_nd against 8
                 dctz_decompress_box_nd calls, wall clock, host buffers)
Every other run also times dctzhip_decompress of the whole shard.  Wall-clock medians go to stdout as one JSON line; for device
times run one --what per process under `rocprofv3 --kernel-trace --stats -- python tools/range_bench.py --what ...`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["index", "range", "one", "full", "dropin", "box", "ndbox", "boxes", "ndboxes"], required=True)
    ap.add_argument("--box", choices=["brick", "zplane", "xplane", "full", "c2"], default="brick")
    ap.add_argument("--via", choices=["box", "ranges", "slice", "list", "loop", "one", "dropin"], default="box")
    ap.add_argument("--n", type=int, default=512, help="edge of the cube")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dctz_amd
    from tests import workloads as W

    if a.what == "dropin":
        return dropin(a, W)
    if a.what == "box":
        return box(a, W)
    if a.what == "ndbox":
        return ndbox(a, W)
    if a.what == "boxes":
        return boxes_dropin(a, W) if a.via == "dropin" else boxes(a, W)
    if a.what == "ndboxes":
        return ndboxes_dropin(a, W) if a.via == "dropin" else ndboxes(a, W)
    ctx = dctz_amd.Context(0)
    x = torch.from_numpy(W.c3(a.n, seed=512)).to(ctx.device)
    n = x.numel()
    eb = 1e-3
    out, info = ctx.compress(x, eb, dctz_amd.EC)
    del x
    full = torch.empty(n, dtype=torch.float64, device=ctx.device)
    idx, tot = ctx.ac_index(out, n)
    assert tot == info.cnt
    lo = n // 2 + 12345
    rng = {"range": (lo, lo + (1 << 21)), "one": (lo, lo + 1), "full": (0, n), "index": None}[a.what]
    dst = None if rng is None else torch.empty(rng[1] - rng[0], dtype=torch.float64, device=ctx.device)

    def t_full():
        ctx.decompress(out, info.cnt, n, torch.float64, eb, info.sf, dctz_amd.EC, dst=full)

    def t_what():
        if rng is None:
            ctx.ac_index(out, n)
        else:
            ctx.decompress_range(out, info.cnt, n, torch.float64, eb, info.sf, rng[0], rng[1], idx, dctz_amd.EC, dst=dst)

    def med(f):
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    for f in (t_full, t_what):                      # warm-up
        f()
    ms_full, ms_what = med(t_full), med(t_what)
    if rng is not None:                             # and the result is the slice of the full decode
        assert torch.equal(dst.view(torch.int64), full[rng[0]:rng[1]].view(torch.int64))
    print(json.dumps({"what": a.what, "n": n, "cnt": info.cnt, "range": rng, "wall_ms_decompress": round(ms_full, 4),
                      "wall_ms_" + a.what: round(ms_what, 4)}))
    ctx.close()


def box(a, W):
    import numpy as np
    import torch
    import dctz_amd

    ctx = dctz_amd.Context(0)
    if a.box == "c2":
        x = torch.from_numpy(np.ascontiguousarray(W.c2(), dtype=np.float32).reshape(-1)).to(ctx.device)
        dims, tdt = (1800, 3600), torch.float32
        lo, hi = (600, 1200), (856, 1712)
    else:
        x = torch.from_numpy(W.c3(a.n, seed=512)).to(ctx.device).reshape(-1)
        e, tdt = a.n, torch.float64
        dims = (e, e, e)
        lo, hi = {"brick": ((224 * e // 512,) * 3, (224 * e // 512 + 64,) * 3), "zplane": ((100, 0, 0), (101, e, e)),
                  "xplane": ((0, 0, 100), (e, e, 101)), "full": ((0, 0, 0), dims)}[a.box]
    n = x.numel()
    eb = 1e-3
    out, info = ctx.compress(x, eb, dctz_amd.EC)
    del x
    full = torch.empty(n, dtype=tdt, device=ctx.device)
    idx, tot = ctx.ac_index(out, n)
    ext = tuple(h - l for l, h in zip(lo, hi))
    dst = torch.empty(ext, dtype=tdt, device=ctx.device)
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    # the box as runs of the flat order: (flat start, length) per row of the box, the fastest dimension as long as it is
    starts = np.ravel_multi_index(np.meshgrid(*[np.arange(l, h) for l, h in zip(lo[:-1], hi[:-1])], [lo[-1]], indexing="ij"), dims).reshape(-1)
    run = ext[-1]
    flat = dst.view(-1)

    def t_full():
        ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def t_box():
        ctx.decompress_box(out, info.cnt, dims, tdt, eb, info.sf, lo, hi, idx, dctz_amd.EC, dst=dst)

    def t_ranges():
        for k, s0 in enumerate(starts):
            ctx.decompress_range(out, info.cnt, n, tdt, eb, info.sf, int(s0), int(s0) + run, idx, dctz_amd.EC, dst=flat[k * run:(k + 1) * run])

    def t_slice():
        t_full()
        dst.copy_(full.view(dims)[sl])

    f_what = {"box": t_box, "ranges": t_ranges, "slice": t_slice}[a.via]
    if a.via == "ranges" and (run * dst.element_size()) % 16:
        raise SystemExit("the runs' outputs are not 16-byte aligned: dctzhip_decompress_range refuses them")

    def med(f, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    for f in (t_full, f_what):                      # warm-up
        f()
    reps = max(3, a.reps // 4) if a.via == "ranges" else a.reps
    ms_full, ms_what = med(t_full, a.reps), med(f_what, reps)
    it = torch.int64 if tdt == torch.float64 else torch.int32
    assert torch.equal(dst.contiguous().view(it), full.view(dims)[sl].contiguous().view(it))
    m = np.zeros(dims, bool)
    m[sl] = True
    fm = np.zeros(-(-n // 4096) * 4096, bool)
    fm[:n] = m.reshape(-1)
    hit = fm.reshape(-1, 4096).any(axis=1)
    t = np.flatnonzero(hit)
    print(json.dumps({"what": "box", "box": a.box, "via": a.via, "n": n, "cnt": info.cnt, "lo": lo, "hi": hi, "rows": int(starts.size),
                      "hit_tiles": int(hit.sum()), "candidate_tiles": int(t[-1] - t[0] + 1), "wall_ms_decompress": round(ms_full, 4),
                      "wall_ms_" + a.via: round(ms_what, 4)}))
    ctx.close()


def lattice(e):
    """The 64 disjoint 64^3 bricks of the cube of edge e (512: at 32 + 128 i in every axis)."""
    at = [(32 + 128 * i) * e // 512 for i in range(4)]
    return [((i, j, k), (i + 64, j + 64, k + 64)) for i in at for j in at for k in at]


def boxes(a, W):
    import numpy as np
    import torch
    import dctz_amd

    if a.via not in ("list", "loop", "one"):
        raise SystemExit("--what boxes takes --via list | loop | one | dropin")
    ctx = dctz_amd.Context(0)
    e, tdt = a.n, torch.float64
    dims = (e, e, e)
    x = torch.from_numpy(W.c3(a.n, seed=512)).to(ctx.device).reshape(-1)
    n = x.numel()
    eb = 1e-3
    out, info = ctx.compress(x, eb, dctz_amd.EC)
    del x
    full = torch.empty(n, dtype=tdt, device=ctx.device)
    idx, tot = ctx.ac_index(out, n)
    bx = [((224 * e // 512,) * 3, (224 * e // 512 + 64,) * 3)] if a.via == "one" else lattice(e)
    dsts = [torch.empty(tuple(h - l for l, h in zip(lo, hi)), dtype=tdt, device=ctx.device) for lo, hi in bx]

    def t_full():
        ctx.decompress(out, info.cnt, n, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def t_list():
        ctx.decompress_boxes(out, info.cnt, dims, tdt, eb, info.sf, bx, idx, dctz_amd.EC, dsts=dsts)

    def t_loop():
        for (lo, hi), d in zip(bx, dsts):
            ctx.decompress_box(out, info.cnt, dims, tdt, eb, info.sf, lo, hi, idx, dctz_amd.EC, dst=d)

    f_what = t_loop if a.via == "loop" else t_list

    def med(f, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    for f in (t_full, f_what):                      # warm-up
        f()
    ms_full, ms_what = med(t_full, a.reps), med(f_what, a.reps)
    for (lo, hi), d in zip(bx, dsts):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        assert torch.equal(d.contiguous().view(torch.int64), full.view(dims)[sl].contiguous().view(torch.int64))
    res = {"what": "boxes", "via": a.via, "n": n, "cnt": info.cnt, "boxes": len(bx), "kernel": ctx.last_kernel(1),
           "wall_ms_decompress": round(ms_full, 4), "wall_ms_" + a.via: round(ms_what, 4)}
    if a.via != "loop":
        res.update(items=ctx.counter(13), grid=ctx.counter(14), bound=ctx.counter(15))
    else:
        res.update(grid_per_call=ctx.counter(11), candidates_per_call=ctx.counter(12))
    print(json.dumps(res))
    ctx.close()


def boxes_dropin(a, W):
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
    lib.dctz_decompress_box.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                        C.POINTER(TVar)]
    lib.dctz_decompress_boxes.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.POINTER(C.POINTER(TVar))]
    e = a.n
    dims = (e, e, e)
    x = W.c3(e, seed=512)
    n = x.size
    z = np.empty(n + (1 << 20), np.float64)
    sz = C.c_size_t(0)
    os.environ["DCTZ_ZLIB_GPU"] = "1"
    assert lib.dctz_compress(C.byref(tv(x)), n, C.byref(sz), C.byref(tv(z)), 1e-3) == 1
    del os.environ["DCTZ_ZLIB_GPU"]
    bx = lattice(e)[21:43:3]                        # 8 bricks from the middle of the lattice
    assert len(bx) == 8
    arr = lambda v: (C.c_size_t * len(v))(*v)
    one = [np.empty(64 ** 3, np.float64) for _ in bx]
    many = [np.empty(64 ** 3, np.float64) for _ in bx]
    tvs = [tv(o) for o in many]
    ptrs = (C.POINTER(TVar) * len(bx))(*[C.pointer(t) for t in tvs])
    los, his = arr([v for lo, hi in bx for v in lo]), arr([v for lo, hi in bx for v in hi])
    d3 = arr(dims)

    def t_loop():
        for (lo, hi), o in zip(bx, one):
            assert lib.dctz_decompress_box(C.byref(tv(z)), 3, d3, arr(lo), arr(hi), C.byref(tv(o))) == 1

    def t_list():
        assert lib.dctz_decompress_boxes(C.byref(tv(z)), 3, d3, len(bx), los, his, ptrs) == 1

    def med(f):
        f()
        ts = []
        for _ in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    ms_loop, ms_list = med(t_loop), med(t_list)
    for o, m in zip(one, many):
        assert np.array_equal(o.view(np.uint64), m.view(np.uint64))
    print(json.dumps({"what": "boxes", "via": "dropin", "n": n, "container_bytes": sz.value, "boxes": len(bx),
                      "wall_ms_8x_dctz_decompress_box": round(ms_loop, 3), "wall_ms_dctz_decompress_boxes": round(ms_list, 3)}))


def ndbox(a, W):
    import numpy as np
    import torch
    import dctz_amd

    if a.box == "c2":
        raise SystemExit("--what ndbox runs the boxes of the cube: brick, zplane, xplane, full")
    ctx = dctz_amd.Context(0)
    e, tdt = a.n, torch.float64
    dims = (e, e, e)
    x = torch.from_numpy(W.c3(a.n, seed=512)).to(ctx.device).reshape(dims)
    lo, hi = {"brick": ((224 * e // 512,) * 3, (224 * e // 512 + 64,) * 3), "zplane": ((100, 0, 0), (101, e, e)),
              "xplane": ((0, 0, 100), (e, e, 101)), "full": ((0, 0, 0), dims)}[a.box]
    eb = 1e-3
    out, info = ctx.compress_nd(x, eb, dctz_amd.EC)
    del x
    nblk = ctx.nd_blocks(dims)
    full = torch.empty(dims, dtype=tdt, device=ctx.device)
    idx, tot = ctx.ac_index(out, 64 * nblk)
    assert tot == info.cnt
    ext = tuple(h - l for l, h in zip(lo, hi))
    dst = torch.empty(ext, dtype=tdt, device=ctx.device)
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))

    def t_full():
        ctx.decompress_nd(out, info.cnt, dims, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def t_box():
        ctx.decompress_box_nd(out, info.cnt, dims, tdt, eb, info.sf, lo, hi, idx, dctz_amd.EC, dst=dst)

    def med(f, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    for f in (t_full, t_box):                       # warm-up
        f()
    ms_full, ms_what = med(t_full, a.reps), med(t_box, a.reps)
    assert torch.equal(dst.contiguous().view(torch.int64), full[sl].contiguous().view(torch.int64))
    nb = [-(-d // 4) for d in dims]                 # the intersecting blocks, 64 to a stream tile
    m = np.zeros(nb, bool)
    m[tuple(slice(l // 4, (h - 1) // 4 + 1) for l, h in zip(lo, hi))] = True
    fm = np.zeros(-(-nblk // 64) * 64, bool)
    fm[:nblk] = m.reshape(-1)
    hit = fm.reshape(-1, 64).any(axis=1)
    t = np.flatnonzero(hit)
    print(json.dumps({"what": "ndbox", "box": a.box, "n": e ** 3, "cnt": info.cnt, "lo": lo, "hi": hi, "tiles": int(hit.size),
                      "hit_tiles": int(hit.sum()), "candidate_tiles": int(t[-1] - t[0] + 1), "grid": ctx.counter(11),
                      "kernel": ctx.last_kernel(1), "wall_ms_decompress_nd": round(ms_full, 4), "wall_ms_box_nd": round(ms_what, 4)}))
    ctx.close()


def ndboxes(a, W):
    import numpy as np
    import torch
    import dctz_amd

    if a.via not in ("list", "loop", "one"):
        raise SystemExit("--what ndboxes takes --via list | loop | one | dropin")
    if a.box == "c2":
        raise SystemExit("--what ndboxes --via one runs the boxes of the cube: brick, zplane, xplane, full")
    ctx = dctz_amd.Context(0)
    e, tdt = a.n, torch.float64
    dims = (e, e, e)
    x = torch.from_numpy(W.c3(a.n, seed=512)).to(ctx.device).reshape(dims)
    eb = 1e-3
    out, info = ctx.compress_nd(x, eb, dctz_amd.EC)
    del x
    nblk = ctx.nd_blocks(dims)
    full = torch.empty(dims, dtype=tdt, device=ctx.device)
    idx, tot = ctx.ac_index(out, 64 * nblk)
    assert tot == info.cnt
    single = {"brick": ((224 * e // 512,) * 3, (224 * e // 512 + 64,) * 3), "zplane": ((100, 0, 0), (101, e, e)),
              "xplane": ((0, 0, 100), (e, e, 101)), "full": ((0, 0, 0), dims)}[a.box]
    bx = [single] if a.via == "one" else lattice(e)
    dsts = [torch.empty(tuple(h - l for l, h in zip(lo, hi)), dtype=tdt, device=ctx.device) for lo, hi in bx]

    def t_full():
        ctx.decompress_nd(out, info.cnt, dims, tdt, eb, info.sf, dctz_amd.EC, dst=full)

    def t_list():
        ctx.decompress_boxes_nd(out, info.cnt, dims, tdt, eb, info.sf, bx, idx, dctz_amd.EC, dsts=dsts)

    def t_loop():
        for (lo, hi), d in zip(bx, dsts):
            ctx.decompress_box_nd(out, info.cnt, dims, tdt, eb, info.sf, lo, hi, idx, dctz_amd.EC, dst=d)

    f_what = t_loop if a.via == "loop" else t_list

    def med(f, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    for f in (t_full, f_what):                      # warm-up
        f()
    ms_full, ms_what = med(t_full, a.reps), med(f_what, a.reps)
    for (lo, hi), d in zip(bx, dsts):
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        assert torch.equal(d.contiguous().view(torch.int64), full[sl].contiguous().view(torch.int64))
    res = {"what": "ndboxes", "via": a.via, "n": e ** 3, "cnt": info.cnt, "boxes": len(bx), "kernel": ctx.last_kernel(1),
           "wall_ms_decompress_nd": round(ms_full, 4), "wall_ms_" + a.via: round(ms_what, 4)}
    if a.via == "one":
        res.update(box=a.box)
    if a.via != "loop":
        res.update(items=ctx.counter(13), grid=ctx.counter(14), bound=ctx.counter(15))
    else:
        res.update(grid_per_call=ctx.counter(11), candidates_per_call=ctx.counter(12))
    print(json.dumps(res))
    ctx.close()


def ndboxes_dropin(a, W):
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
    lib.dctz_decompress_box_nd.argtypes = [C.POINTER(TVar), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(TVar)]
    lib.dctz_decompress_boxes_nd.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
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
    bx = lattice(e)[21:43:3]                        # 8 bricks from the middle of the lattice
    assert len(bx) == 8
    one = [np.empty(64 ** 3, np.float64) for _ in bx]
    many = [np.empty(64 ** 3, np.float64) for _ in bx]
    tvs = [tv(o) for o in many]
    ptrs = (C.POINTER(TVar) * len(bx))(*[C.pointer(t) for t in tvs])
    los, his = arr([v for lo, hi in bx for v in lo]), arr([v for lo, hi in bx for v in hi])

    def t_loop():
        for (lo, hi), o in zip(bx, one):
            assert lib.dctz_decompress_box_nd(C.byref(tv(z)), arr(lo), arr(hi), C.byref(tv(o))) == 1

    def t_list():
        assert lib.dctz_decompress_boxes_nd(C.byref(tv(z)), len(bx), los, his, ptrs) == 1

    def med(f):
        f()
        ts = []
        for _ in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    ms_loop, ms_list = med(t_loop), med(t_list)
    for o, m in zip(one, many):
        assert np.array_equal(o.view(np.uint64), m.view(np.uint64))
    print(json.dumps({"what": "ndboxes", "via": "dropin", "n": n, "container_bytes": sz.value, "boxes": len(bx),
                      "wall_ms_8x_dctz_decompress_box_nd": round(ms_loop, 3), "wall_ms_dctz_decompress_boxes_nd": round(ms_list, 3)}))


def dropin(a, W):
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
    lib.dctz_decompress.argtypes = [C.POINTER(TVar), C.POINTER(TVar)]
    lib.dctz_decompress_range.argtypes = [C.POINTER(TVar), C.c_size_t, C.c_size_t, C.POINTER(TVar)]
    x = W.c3(a.n, seed=512)
    n = x.size
    z = np.empty(n + (1 << 20), np.float64)
    sz = C.c_size_t(0)
    os.environ["DCTZ_ZLIB_GPU"] = "1"
    assert lib.dctz_compress(C.byref(tv(x)), n, C.byref(sz), C.byref(tv(z)), 1e-3) == 1
    del os.environ["DCTZ_ZLIB_GPU"]
    full = np.empty(n, np.float64)
    lo = n // 2 + 12345
    hi = lo + (1 << 21)
    part = np.empty(hi - lo, np.float64)

    def med(f):
        f()
        ts = []
        for _ in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    ms_full = med(lambda: lib.dctz_decompress(C.byref(tv(z)), C.byref(tv(full))))
    ms_part = med(lambda: lib.dctz_decompress_range(C.byref(tv(z)), lo, hi, C.byref(tv(part))))
    assert np.array_equal(part.view(np.uint64), full[lo:hi].view(np.uint64))
    print(json.dumps({"what": "dropin", "n": n, "container_bytes": sz.value, "range": [lo, hi],
                      "wall_ms_dctz_decompress": round(ms_full, 3), "wall_ms_dctz_decompress_range": round(ms_part, 3)}))


if __name__ == "__main__":
    main()
