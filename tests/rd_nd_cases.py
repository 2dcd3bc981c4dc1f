"""Inputs of the tiled rate-distortion probe's tests (dctzhip_rd_probe_nd, dctzhip_compress_psnr_nd) and the numpy statement of
its prediction, shared by the CPU and the GPU files.

The prediction, per bound: the coefficients of oracle.compress_nd(..., want_coef=True) against the decoder's value for each of
them -- the bin centre (floor(q) - 127) * bw, the float truncation for bin 255 and for the DC -- squared and summed over all 64
places of every tile, times sf^2; then, for the tiles that hang over an extent, the inverse transform of those coefficient
errors (oracle.dct_inv with the geometry) squared at the padded places is taken out again."""
import functools

import numpy as np

from oracle import oracle as O
from tests import workloads as W

# 16 bounds from the smallest accepted one to 1 (tests/test_gpu_rd_probe.py: EBS)
EBS = [1e-6, 2e-6, 5e-6, 1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0]
SSE_RTOL_F64 = 1e-8                  # tests/test_gpu_rd_probe.py
F32_RTOL = 1e-3

SMALL_2D = [(64, 128), (203, 517), (9, 4099), (8, 8), (3, 5), (64, 130)]
SMALL_3D = [(64, 64, 64), (37, 42, 63), (5, 6, 7), (4, 4, 4)]
SMALL = SMALL_2D + SMALL_3D
BIG = [(2050, 2051), (164, 161, 162)]            # past one grid round of the probe (1032 / 1077 stream tiles); fp64 only
# (input, type, bound) pairs at which the REFERENCE ALONE -- the numpy statement below against the oracle's decode -- misses the
# SSE rule; they are left out of the SSE checks on the CPU and on the GPU (the counts, the range and everything else are still
# checked there).  All are one-tile arrays: a single block has nothing to average the inverse transform's rounding over.
#   (8, 8) fp64, 1e-6 .. 1e-5: all 63 coefficients stored exactly, the error is the float truncation alone (SSE 2.8e-14);
#                              relative miss 1.9e-8
#   (3, 5) fp64, 1e-6 .. 2e-5: the same (SSE 1.6e-15); relative miss 1.4e-8
#   (3, 5) fp32, 2e-4:         relative miss 1.27e-3 of an SSE of 3.8e-8, the rounding slack of 15 elements is 4.9e-12
SSE_DROPPED = ({((8, 8), "float64", eb) for eb in (1e-6, 2e-6, 5e-6, 1e-5)}
               | {((3, 5), "float64", eb) for eb in (1e-6, 2e-6, 5e-6, 1e-5, 2e-5)}
               | {((3, 5), "float32", 2e-4)})
TARGET_SHAPES = [(203, 517), (37, 42, 63)]
TARGETS = (40.0, 60.0, 80.0, 100.0)


@functools.lru_cache(maxsize=None)
def _base(which):
    if which == "c2":
        a = W.c2().reshape(1800, 3600) * 37
    elif which == "c3":
        a = W.c3(64).reshape(64, 64, 64)
    else:
        a = W.c3(168)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _array(shape, dtype):
    if shape in BIG:
        a = _base("big")[:int(np.prod(shape))].reshape(shape)
    elif len(shape) == 2 and shape[1] > 3600:                  # wider than the field: its first prod(shape) elements
        a = _base("c2").reshape(-1)[:int(np.prod(shape))].reshape(shape)
    else:
        a = _base("c2" if len(shape) == 2 else "c3")[tuple(slice(0, d) for d in shape)]
    a = np.ascontiguousarray(a).astype(dtype)
    a.setflags(write=False)
    return a


def array(shape, dtype):
    """The input of `shape` in `dtype` (read-only, shared)."""
    return _array(tuple(shape), np.dtype(dtype))


def f32_slack(x):
    """The fp32 rule's bound on the share of the reconstruction's own rounding (tests/test_gpu_rd_probe.py)."""
    return x.size * (8 * 2.0 ** -24 * float(np.abs(x).max())) ** 2


def sse_checked(shape, dtype, eb):
    return (tuple(shape), np.dtype(dtype).name, eb) not in SSE_DROPPED


def sse_ok(pred, meas, x):
    if x.dtype == np.float64:
        return abs(pred - meas) <= SSE_RTOL_F64 * meas
    return abs(pred - meas) <= F32_RTOL * meas + f32_slack(x)


def nd_blocks(shape):
    e = O.GEOM_EDGE[len(shape)]
    return int(np.prod([(d + e - 1) // e for d in shape]))


def real_lin(shape):
    """Per stream position of the block-linear layout: does it lie inside the array?"""
    e = O.GEOM_EDGE[len(shape)]
    m = np.pad(np.ones(shape, np.uint8), [(0, (-d) % e) for d in shape], mode="constant")
    return O.nd_gather(m).astype(bool)


def measured_sse(x, r):
    """calc_psnr's sum (util.c:72-73 / :88-89): difference and square in the data type, summed in double."""
    d = x - r.astype(x.dtype)
    return float(np.sum((d * d).astype(np.float64)))


def psnr_of(x, sse):
    return 20.0 * np.log10((float(x.max()) - float(x.min())) / np.sqrt(sse / x.size))


def predict(x, eb):
    """(cnt, predicted SSE over the array's elements, predicted SSE over all stream positions, the oracle's Compressed)."""
    T = x.dtype.type
    c = O.compress_nd(x, eb, want_coef=True)
    coef = c.coef
    bw, rmin = T(eb * 2.0 * 1.0), T(-(255) * (eb * 1.0))
    q = (coef - rmin) / bw
    centre = (np.floor(q) - T(127)) * bw
    trunc = coef.astype(np.float32).astype(x.dtype)
    exact = c.bin_index == 255
    dec = np.where(exact, trunc, centre)
    dec[0::64] = trunc[0::64]                                  # the DC travels as a float
    sf2 = float(T(c.sf)) ** 2
    err = coef.astype(np.float64) - dec.astype(np.float64)
    total = float(np.sum(err * err))
    real = real_lin(x.shape)
    edge = ~real.reshape(-1, 64).all(axis=1)
    share = 0.0
    if edge.any():
        e_t = (coef - dec).reshape(-1, 64)[edge]
        pad = ~real.reshape(-1, 64)[edge]
        for b in range(e_t.shape[0]):                          # (the oracle's N-D transform takes one block a call)
            inv = O.dct_inv(e_t[b], O.geom_impl(x.ndim)).astype(np.float64)
            share += float(np.sum((inv * inv)[pad[b]]))
    cnt = int(np.count_nonzero(exact.reshape(-1, 64)[:, 1:]))
    assert cnt == c.cnt
    return cnt, sf2 * (total - share), sf2 * total, c


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, eb):
    x = _array(shape, dtype)
    cnt, sse, sse_all, c = predict(x, eb)
    meas = measured_sse(x, O.decompress_nd(c, shape))
    lin = O.decompress(c, O.geom_impl(len(shape)))
    g = O.nd_gather(x)
    padded = measured_sse(g, lin)
    return {"cnt": cnt, "pred": sse, "pred_padded_layout": sse_all, "meas": meas, "meas_padded_layout": padded, "sf": c.sf}


def reference(shape, dtype, eb):
    """The numpy prediction and the oracle's own measurement for one (input, bound), computed once."""
    return _reference(tuple(shape), np.dtype(dtype), float(eb))


def grid():
    """The 61 candidate bounds of the target-PSNR calls (include/dctz_hip.h)."""
    g = [float(f"{m}e{e}") for e in range(-6, 0) for m in ("1", "1.25", "1.5", "2", "2.5", "3", "4", "5", "6", "8")]
    return g + [1.0]


def search(shape, dtype, target):
    """The contract's choice from the numpy predictions: index into grid(), or None when no point is predicted to reach it."""
    g = grid()
    x = array(shape, dtype)
    pred = lambda i: psnr_of(x, reference(shape, dtype, g[i])["pred"])
    at = None
    for d in range(6, -1, -1):
        if pred(10 * d) >= target:
            at = 10 * d
            break
    if at is None:
        return None
    if at < len(g) - 1:
        for i in range(8, -1, -1):
            if pred(at + 1 + i) >= target:
                at = at + 1 + i
                break
    return at


def measured_psnr(shape, dtype, eb):
    x = array(shape, dtype)
    c = O.compress_nd(x, eb)
    return O.psnr(x, O.decompress_nd(c, shape))["psnr"]
