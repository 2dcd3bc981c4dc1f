"""Compression of a tiled array to a target PSNR (dctzhip_compress_psnr_nd, dctz_compress_psnr_nd): the returned streams measure
at least the target over the array's own elements, are those of an ordinary compress_nd at the chosen bound, and that bound is
the largest point of the grid that measures at the target (tests/test_rd_probe_nd_cases_cpu.py states the same search on the
CPU, for the same inputs and targets)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import rd_nd_cases as R
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu
GRID = H.psnr_grid()
LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dctz_amd", "lib")
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


def _measured(ctx, x, d, eb):
    out, info = ctx.compress_nd(d, eb)
    r = ctx.decompress_nd(out, info.cnt, x.shape, _tdt(x.dtype), eb, info.sf).cpu().numpy()
    return O.psnr(x, r)["psnr"]


def test_grid_is_the_cpu_files():
    assert GRID == R.grid()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", R.TARGET_SHAPES, ids=_ids)
def test_targets(ctx, shape, dtype):
    x = R.array(shape, dtype)
    d = _dev(ctx, x)
    for target in R.TARGETS:
        out, info, eb, psnr = ctx.compress_psnr_nd(d, target)
        assert eb in GRID
        r = ctx.decompress_nd(out, info.cnt, shape, _tdt(dtype), eb, info.sf).cpu().numpy()
        got = O.psnr(x, r)["psnr"]
        assert got >= target, (shape, target, eb, got)
        assert abs(got - psnr) < 1e-9 * abs(got)
        ref, rinfo = ctx.compress_nd(d, eb)
        assert rinfo.cnt == info.cnt and rinfo.sf == info.sf
        for k in ("bin_index", "dc"):
            assert np.array_equal(out[k].cpu().numpy(), ref[k].cpu().numpy())
        assert np.array_equal(out["ac_exact"][:info.cnt].cpu().numpy().view(np.uint32),
                              ref["ac_exact"][:info.cnt].cpu().numpy().view(np.uint32))
        c = O.compress_nd(x, eb)
        assert c.cnt == info.cnt and c.sf == info.sf and np.array_equal(out["bin_index"].cpu().numpy(), c.bin_index)
        assert np.array_equal(out["dc"].cpu().numpy().view(np.uint32), c.dc.view(np.uint32))
        assert np.array_equal(out["ac_exact"][:c.cnt].cpu().numpy().view(np.uint32), c.ac_exact.view(np.uint32))
        i = GRID.index(eb)
        if i + 1 < len(GRID):
            assert _measured(ctx, x, d, GRID[i + 1]) < target, (shape, target, eb)
        assert np.array_equal(x, d.cpu().numpy())           # d_in not modified


def _fill(out):
    for v in out.values():
        v.view(__import__("torch").uint8).fill_(0xA5)


def _untouched(out):
    return all(bool((v.view(__import__("torch").uint8) == 0xA5).all()) for v in out.values())


def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    xn = R.array((203, 517), np.float64).copy()
    xn[77, 123] = np.nan
    cases = [(R.array((37, 42, 63), np.float32), 400.0, H.E_BOUND),
             (np.full((21, 35), 2.5, np.float64), 40.0, H.E_ARG),
             (xn, 40.0, H.E_ARG),
             (R.array((203, 517), np.float64), float("inf"), H.E_ARG)]
    for x, target, code in cases:
        d = _dev(ctx, x)
        out = ctx.alloc_outputs(ctx.nd_blocks(x.shape) * 64, _tdt(x.dtype))
        _fill(out)
        info, eb, ps = H.CompressInfo(), C.c_double(-7.0), C.c_double(-7.0)
        dims = (C.c_size_t * x.ndim)(*x.shape)
        rc = ctx.lib.dctzhip_compress_psnr_nd(ctx.h, d.data_ptr(), x.ndim, dims, H.F64 if x.dtype == np.float64 else H.F32, target,
                                              out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                              C.byref(info), C.byref(eb), C.byref(ps))
        torch.cuda.synchronize()
        assert rc == code, (x.dtype, target, rc)
        assert _untouched(out) and eb.value == -7.0 and ps.value == -7.0
    # overlapping buffers: the DC stream inside the bin ids
    x = R.array((203, 517), np.float64)
    d = _dev(ctx, x)
    out = ctx.alloc_outputs(ctx.nd_blocks(x.shape) * 64, _tdt(x.dtype))
    _fill(out)
    info, eb, ps = H.CompressInfo(), C.c_double(-7.0), C.c_double(-7.0)
    rc = ctx.lib.dctzhip_compress_psnr_nd(ctx.h, d.data_ptr(), 2, (C.c_size_t * 2)(203, 517), H.F64, 60.0, out["bin_index"].data_ptr(),
                                          out["bin_index"].data_ptr() + 64, out["ac_exact"].data_ptr(), C.byref(info), C.byref(eb), C.byref(ps))
    torch.cuda.synchronize()
    assert rc == H.E_ARG and _untouched(out) and eb.value == -7.0


def test_step_down_path(ctx):
    x = R.array((203, 517), np.float64)
    d = _dev(ctx, x)
    _, _, eb0, _ = ctx.compress_psnr_nd(d, 70.0)
    before = ctx.counter(10)
    ctx.knob(3, 1000)                                       # predictions 30 dB too optimistic
    try:
        out, info, eb, psnr = ctx.compress_psnr_nd(d, 70.0)
    finally:
        ctx.knob(3, 0)
    assert ctx.counter(10) > before
    assert eb == eb0 and psnr >= 70.0                       # the measurement walks down to the same point
    assert _measured(ctx, x, d, eb) >= 70.0
    steps = ctx.counter(10)
    _, _, eb1, _ = ctx.compress_psnr_nd(d, 70.0)
    assert eb1 == eb0 and ctx.counter(10) == steps


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


def _lib(mode):
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIBDIR, f"libdctz-{mode}.so"))
    ps = C.POINTER(C.c_size_t)
    lib.dctz_compress.argtypes = [C.POINTER(TVar), C.c_int, ps, C.POINTER(TVar), C.c_double]
    lib.dctz_compress_psnr_nd.argtypes = [C.POINTER(TVar), C.c_int, ps, ps, C.POINTER(TVar), C.c_double, C.POINTER(C.c_double)]
    lib.dctz_set_block_dims.argtypes = [C.c_int, ps]
    lib.dctz_decompress.argtypes = [C.POINTER(TVar), C.POINTER(TVar)]
    return lib


def _tvar(arr):
    v = TVar()
    v.datatype = 1 if arr.dtype == np.float64 else 0
    if arr.dtype == np.float64:
        v.buf.d = arr.ctypes.data_as(C.POINTER(C.c_double))
    else:
        v.buf.f = arr.ctypes.data_as(C.POINTER(C.c_float))
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", R.TARGET_SHAPES, ids=_ids)
def test_dropin_container_is_dctz_compress_in_tiles_at_the_chosen_bound(shape, dtype):
    lib = _lib("ec")
    x0 = R.array(shape, dtype)
    a, b = x0.copy(), x0.copy()
    za, zb = np.zeros(x0.nbytes * 3 + 4096, np.uint8), np.zeros(x0.nbytes * 3 + 4096, np.uint8)
    va, vb, vza, vzb = _tvar(a), _tvar(b), TVar(), TVar()
    vza.datatype = vzb.datatype = va.datatype
    vza.buf.d = za.ctypes.data_as(C.POINTER(C.c_double))
    vzb.buf.d = zb.ctypes.data_as(C.POINTER(C.c_double))
    sa, sb, eb = C.c_size_t(0), C.c_size_t(0), C.c_double(0.0)
    dims = (C.c_size_t * len(shape))(*shape)
    assert lib.dctz_compress_psnr_nd(C.byref(va), len(shape), dims, C.byref(sa), C.byref(vza), 65.0, C.byref(eb)) == 1
    assert eb.value in GRID
    assert lib.dctz_set_block_dims(len(shape), dims) == 0
    assert lib.dctz_compress(C.byref(vb), x0.size, C.byref(sb), C.byref(vzb), eb.value) == 1
    assert sa.value == sb.value and np.array_equal(za[:sa.value], zb[:sb.value])
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))          # the in-place x /= sf, as dctz_compress leaves it
    r = np.zeros_like(x0)
    vr = _tvar(r)
    lib.dctz_decompress(C.byref(vza), C.byref(vr))
    assert O.psnr(x0, r)["psnr"] >= 65.0


def test_dropin_qt_refuses():
    lib = _lib("qt")
    x0 = R.array((203, 517), np.float64)
    a = x0.copy()
    z = np.full(x0.nbytes * 2, 0x5A, np.uint8)
    va, vz = _tvar(a), TVar()
    vz.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    size, eb = C.c_size_t(12345), C.c_double(-1.0)
    assert lib.dctz_compress_psnr_nd(C.byref(va), 2, (C.c_size_t * 2)(203, 517), C.byref(size), C.byref(vz), 60.0, C.byref(eb)) < 0
    assert size.value == 12345 and eb.value == -1.0 and np.array_equal(a, x0) and (z == 0x5A).all()
