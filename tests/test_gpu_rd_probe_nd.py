"""The rate-distortion probe of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (dctzhip_rd_probe_nd, dctz_kernels_ndrd.hip).

Bars: the counts are those of a real compress_nd (in place or through its gather pass) and of the oracle exactly; the predicted
SSE covers the array's own elements -- the edge padding of the streams enters no field -- and is the measured one up to the
rounding of the inverse transform (the rules of tests/test_gpu_rd_probe.py; tests/test_rd_probe_nd_cases_cpu.py holds the
reference alone to them); the range is dctzhip_psnr_terms' exactly; results are bitwise reproducible and do not depend on the
other bounds of the call."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import rd_nd_cases as R
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu
EBS = R.EBS
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)       # (a copy: the shared inputs are read-only)


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _cases():
    return [(s, dt) for s in R.SMALL for dt in (np.float64, np.float32)] + [(s, np.float64) for s in R.BIG]


@pytest.mark.parametrize("shape,dtype", _cases(), ids=_ids)
def test_counts_equal_compress_nd_and_oracle(ctx, shape, dtype):
    x = R.array(shape, dtype)
    d = _dev(ctx, x)
    pts, _ = ctx.rd_probe_nd(d, EBS)
    nblk = R.nd_blocks(shape)
    assert nblk == ctx.nd_blocks(shape)
    for eb, p in zip(EBS, pts):
        _, info = ctx.compress_nd(d, eb)
        want = O.compress_nd(x, eb).cnt
        assert p["error_bound"] == eb
        assert p["cnt"] == info.cnt == want, (shape, eb, p["cnt"], info.cnt, want)
        assert p["raw_bytes"] == 64 * nblk + 4 * nblk + 4 * info.cnt + 56 + 16


@pytest.mark.parametrize("shape,dtype", _cases(), ids=_ids)
def test_predicted_sse_and_range_match_the_measurement(ctx, shape, dtype):
    x = R.array(shape, dtype)
    d = _dev(ctx, x)
    pts, rng = ctx.rd_probe_nd(d, EBS)
    worst = 0.0
    for eb, p in zip(EBS, pts):
        out, info = ctx.compress_nd(d, eb)
        r = ctx.decompress_nd(out, info.cnt, shape, _tdt(dtype), eb, info.sf)
        t = ctx.psnr_terms(d.reshape(-1), r.reshape(-1))
        assert rng == (t[0], t[1]), (shape, rng, t[:2])
        if not R.sse_checked(shape, dtype, eb):
            continue
        miss = abs(p["sse"] - t[3])
        print(f"{shape} {np.dtype(dtype).name} eb {eb:g}: predicted {p['sse']:.12e} measured {t[3]:.12e} relative miss {miss / t[3]:.3e}")
        assert R.sse_ok(p["sse"], t[3], x), (shape, eb, p["sse"], t[3], miss / t[3])
        if np.dtype(dtype) == np.float64:
            psnr = 20 * np.log10((t[1] - t[0]) / np.sqrt(t[3] / x.size))
            assert abs(p["psnr"] - psnr) <= 1e-7
            worst = max(worst, miss / t[3])
        elif miss > R.f32_slack(x):
            worst = max(worst, miss / t[3])
    print(f"worst relative SSE miss, {shape} {np.dtype(dtype).name} (fp32: where it exceeds the rounding share): {worst:.3e}")


@pytest.mark.parametrize("shape", [(9, 4099), (5, 6, 7)], ids=_ids)
def test_the_padded_share_is_taken_out(ctx, shape):
    ref = R.reference(shape, np.float64, 1e-3)
    pts, _ = ctx.rd_probe_nd(_dev(ctx, R.array(shape, np.float64)), [1e-3])
    print(f"{shape}: predicted {pts[0]['sse']:.6e}, SSE of the padded layout {ref['meas_padded_layout']:.6e}, "
          f"ratio {pts[0]['sse'] / ref['meas_padded_layout']:.3f}")
    assert pts[0]["sse"] < 0.97 * ref["meas_padded_layout"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(203, 517), (37, 42, 63)], ids=_ids)
def test_reproducible_and_independent_of_the_other_bounds(ctx, shape, dtype):
    x = R.array(shape, dtype)
    d = _dev(ctx, x)
    a, ra = ctx.rd_probe_nd(d, EBS)
    b, rb = ctx.rd_probe_nd(d, EBS)
    assert a == b and ra == rb                              # bitwise: Python floats compare by value, and -0.0 / NaN do not occur
    perm = list(np.random.default_rng(5).permutation(len(EBS)))
    c, _ = ctx.rd_probe_nd(d, [EBS[i] for i in perm])
    for j, i in enumerate(perm):
        assert c[j] == a[i]
    dup = [EBS[3], EBS[3], EBS[9], EBS[3]]
    e, _ = ctx.rd_probe_nd(d, dup)
    assert e == [a[3], a[3], a[9], a[3]]
    one, _ = ctx.rd_probe_nd(d, [EBS[7]])
    assert one == [a[7]]
    assert np.array_equal(x, d.cpu().numpy())               # d_in not modified


@pytest.mark.parametrize("shape,at", [((203, 517), (100, 300)), ((37, 42, 63), (36, 41, 62))], ids=_ids)
def test_a_nan_in_the_array(ctx, shape, at):
    x = R.array(shape, np.float64).copy()
    x[at] = np.nan
    d = _dev(ctx, x)
    pts, rng = ctx.rd_probe_nd(d, [1e-3, 1e-2])
    for eb, p in zip([1e-3, 1e-2], pts):
        _, info = ctx.compress_nd(d, eb)
        assert p["cnt"] == info.cnt
        assert np.isnan(p["sse"])
    assert rng == (float(np.nanmin(x)), float(np.nanmax(x)))


def test_refusals(ctx):
    x = _dev(ctx, R.array((203, 517), np.float64))
    lib, h = ctx.lib, ctx.h
    pts = (H.RdPoint * 17)()
    rng = (C.c_double * 2)()

    def call(k, ebs, nd=2, dims=(203, 517), ptr=x.data_ptr(), p=pts, hh=h):
        e = (C.c_double * max(len(ebs), 1))(*ebs) if ebs is not None else None
        dd = (C.c_size_t * len(dims))(*dims) if dims is not None else None
        return lib.dctzhip_rd_probe_nd(hh, ptr, nd, dd, H.F64, k, e, p, rng)

    assert call(0, [1e-3]) == H.E_ARG
    assert call(17, [1e-3] * 17) == H.E_ARG
    assert call(2, [1e-3, 5e-7]) == H.E_BOUND
    assert call(1, [1e-3], nd=1, dims=(203 * 517,)) == H.E_ARG
    assert call(1, [1e-3], nd=4, dims=(7, 29, 11, 47)) == H.E_ARG
    assert call(1, [1e-3], dims=(0, 517)) == H.E_ARG
    assert call(1, [1e-3], dims=(203, 0)) == H.E_ARG
    assert call(1, [1e-3], dims=None) == H.E_ARG
    assert call(1, [1e-3], ptr=None) == H.E_ARG
    assert call(1, None) == H.E_ARG
    assert call(1, [1e-3], p=None) == H.E_ARG
    assert call(1, [1e-3], hh=None) == H.E_ARG
    assert call(16, [1e-3] * 16) == H.OK                   # the limit itself
