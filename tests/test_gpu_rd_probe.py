"""The rate-distortion probe (dctzhip_rd_probe, dctz_kernels_rd.hip): per error bound the exact tot_AC_exact_count and
the predicted squared error of the reconstruction, from one read of the array.

Bars: the counts are those of a real compress (and of the oracle) exactly; the predicted SSE is the measured one up to
the rounding of the inverse transform; the range is dctzhip_psnr_terms' exactly; results are bitwise reproducible and
do not depend on the other bounds of the call."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

# 16 bounds from the smallest accepted one to 1
EBS = [1e-6, 2e-6, 5e-6, 1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0]

# fp64: |predicted - measured| / measured over every bound and workload below; the derivation expects ~1e-9 (the inverse
# transform's rounding against the quantisation error), the worst case observed on an MI355X was 2.4e-10.
SSE_RTOL_F64 = 1e-8
# fp32: the reconstruction is rounded to float, element by element (relative 2^-24 of the data) and inside the inverse
# transform; the prediction does not see that error.  At the small bounds it dominates -- observed on an MI355X: at 1e-6 on
# `ragged` (|x| <= 48, sf = 10) the prediction was 1.15e-9 against a measured 4.26e-7 -- so fp32 is held to the quantisation
# part: |predicted - measured| <= F32_RTOL * measured + n * (8 * 2^-24 * max|x|)^2, the second term a bound on the
# rounding's share.
F32_RTOL = 1e-3


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _workloads(dtype):
    return [("ragged", W.ragged(64 * 777 + 45, dtype, scale=37.0)),
            ("c2", W.c2().astype(dtype)),
            ("big", W.ragged((1 << 24) + 29, dtype, seed=11, scale=5.0))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_counts_equal_compress_and_oracle(ctx, dtype):
    for name, x in _workloads(dtype):
        d = _dev(ctx, x)
        pts, _ = ctx.rd_probe(d, EBS)
        for eb, p in zip(EBS, pts):
            _, info = ctx.compress(d, eb)
            want = O.compress(x, eb, H.EC, O.FAST).cnt
            assert p["error_bound"] == eb
            assert p["cnt"] == info.cnt == want, (name, eb, p["cnt"], info.cnt, want)
            nblk = (x.size + 63) // 64
            assert p["raw_bytes"] == x.size + 4 * nblk + 4 * info.cnt + 56


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_predicted_sse_matches_measurement(ctx, dtype):
    worst = 0.0
    for name, x in _workloads(dtype):
        slack = 0.0 if dtype == np.float64 else x.size * (8 * 2.0 ** -24 * float(np.abs(x).max())) ** 2
        d = _dev(ctx, x)
        pts, rng = ctx.rd_probe(d, EBS)
        for eb, p in zip(EBS, pts):
            out, info = ctx.compress(d, eb)
            r = ctx.decompress(out, info.cnt, x.size, _tdt(dtype), eb, info.sf)
            t = ctx.psnr_terms(d, r)
            assert rng == (t[0], t[1]), (name, rng, t[:2])
            miss = abs(p["sse"] - t[3])
            if dtype == np.float64:
                assert miss <= SSE_RTOL_F64 * t[3], (name, eb, p["sse"], t[3], miss / t[3])
                psnr = 20 * np.log10((t[1] - t[0]) / np.sqrt(t[3] / x.size))
                assert abs(p["psnr"] - psnr) <= 1e-7
            else:
                assert miss <= F32_RTOL * t[3] + slack, (name, eb, p["sse"], t[3], miss / t[3], slack)
            if miss > slack:
                worst = max(worst, miss / t[3])
    print(f"worst relative SSE miss, {np.dtype(dtype).name} (fp32: where it exceeds the rounding share): {worst:.3e}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reproducible_and_independent_of_the_other_bounds(ctx, dtype):
    x = W.ragged((1 << 22) + 64 * 5 + 3, dtype, seed=3, scale=91.0)
    d = _dev(ctx, x)
    a, ra = ctx.rd_probe(d, EBS)
    b, rb = ctx.rd_probe(d, EBS)
    assert a == b and ra == rb                              # bitwise: Python floats compare by value, and -0.0 / NaN do not occur
    perm = list(np.random.default_rng(5).permutation(len(EBS)))
    c, _ = ctx.rd_probe(d, [EBS[i] for i in perm])
    for j, i in enumerate(perm):
        assert c[j] == a[i]
    dup = [EBS[3], EBS[3], EBS[9], EBS[3]]
    e, _ = ctx.rd_probe(d, dup)
    assert e == [a[3], a[3], a[9], a[3]]
    one, _ = ctx.rd_probe(d, [EBS[7]])
    assert one == [a[7]]
    assert np.array_equal(_dev(ctx, x).cpu().numpy(), d.cpu().numpy())        # d_in not modified


def test_refusals(ctx):
    x = _dev(ctx, W.ragged(5000, np.float64))
    lib, h = ctx.lib, ctx.h
    pts = (H.RdPoint * 17)()
    rng = (C.c_double * 2)()

    def call(k, ebs, n=x.numel(), ptr=x.data_ptr(), p=pts):
        e = (C.c_double * max(len(ebs), 1))(*ebs) if ebs is not None else None
        return lib.dctzhip_rd_probe(h, ptr, n, H.F64, k, e, p, rng)

    assert call(0, [1e-3]) == H.E_ARG
    assert call(17, [1e-3] * 17) == H.E_ARG
    assert call(2, [1e-3, 5e-7]) == H.E_BOUND
    assert call(1, [1e-3], n=0) == H.E_ARG
    assert call(1, [1e-3], ptr=None) == H.E_ARG
    assert call(1, None) == H.E_ARG
    assert call(1, [1e-3], p=None) == H.E_ARG
    assert lib.dctzhip_rd_probe(None, x.data_ptr(), x.numel(), H.F64, 1, (C.c_double * 1)(1e-3), pts, rng) == H.E_ARG
    assert call(16, [1e-3] * 16) == H.OK                   # the limit itself
