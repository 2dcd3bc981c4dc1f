"""CPU-side checks of the tiled rate-distortion calls: dctzhip_rd_probe_nd and dctzhip_compress_psnr_nd are exported by
libdctzhip.so with the documented argument types, dctz_compress_psnr_nd by both drop-in libraries; the prototypes stand in the
headers and compile; the device ABI refuses a NULL context before it touches a GPU (the other refusals need a context:
tests/test_gpu_rd_probe_nd.py and tests/test_gpu_psnr_target_nd.py make them); the drop-in refuses the QT build, a shape and a
pending request before it asks for a device (there is none here: a call that went on would end the process)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
CALLS = ("dctzhip_rd_probe_nd", "dctzhip_compress_psnr_nd")
DROPIN = ("dctz_compress_psnr_nd",)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not all(os.path.exists(os.path.join(LIB, f)) for f in ("libdctzhip.so", "libdctz-ec.so", "libdctz-qt.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, so)], text=True)
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return " ".join(f.read().split())


def test_shim_exports_the_calls():
    assert set(CALLS) <= _exported("libdctzhip.so")
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    for name in CALLS:
        assert hasattr(lib, name)
    for name in ("rd_probe_nd", "compress_psnr_nd"):
        assert hasattr(H.Context, name)


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert set(DROPIN) <= _exported(so)


def test_argument_types_and_prototypes(tmp_path):
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    vp, ps, pd = C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_double)
    assert lib.dctzhip_rd_probe_nd.restype is C.c_int
    assert lib.dctzhip_rd_probe_nd.argtypes == [vp, vp, C.c_int, ps, C.c_int, C.c_int, pd, C.POINTER(H.RdPoint), pd]
    assert lib.dctzhip_compress_psnr_nd.restype is C.c_int
    assert lib.dctzhip_compress_psnr_nd.argtypes == [vp, vp, C.c_int, ps, C.c_int, C.c_double, vp, vp, vp, C.POINTER(H.CompressInfo), pd, pd]
    hdr = _header("dctz_hip.h")
    assert ("int dctzhip_rd_probe_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype, int k, "
            "const double *error_bounds, dctzhip_rd_point *pts, double range[2]);") in hdr
    assert ("int dctzhip_compress_psnr_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype, "
            "double target_psnr, void *d_bin_index, float *d_dc, float *d_ac_exact, dctzhip_cinfo *info, "
            "double *error_bound_used, double *psnr_measured);") in hdr
    hdr = _header("dctz.h")
    assert ("int dctz_compress_psnr_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, "
            "double target_psnr, double *error_bound_used);") in hdr
    # the flat call keeps refusing tiled requests, and says so
    assert "flat blocks only" in hdr and "int dctz_compress_psnr(t_var *var, int N," in hdr
    # the prototypes compile, and calls written after the documented signatures compile against them without a warning
    src = tmp_path / "proto.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "dctz_hip.h"\n#include "dctz.h"\n'
                   'int use(dctzhip_ctx *c, void *p, const size_t *dims, const double *ebs, dctzhip_rd_point *pts, double *rng,\n'
                   '        dctzhip_cinfo *info, t_var *v, size_t *sz, double *eb) {\n'
                   '  int (*a)(dctzhip_ctx *, const void *, int, const size_t *, int, int, const double *, dctzhip_rd_point *, double *) = dctzhip_rd_probe_nd;\n'
                   '  int (*b)(t_var *, int, const size_t *, size_t *, t_var *, double, double *) = dctz_compress_psnr_nd;\n'
                   '  return a(c, p, 2, dims, DCTZHIP_F64, DCTZHIP_RD_MAXK, ebs, pts, rng)\n'
                   '       + dctzhip_compress_psnr_nd(c, p, 3, dims, DCTZHIP_F32, 60.0, p, (float *)p, (float *)p, info, eb, eb)\n'
                   '       + b(v, 2, dims, sz, v, 60.0, eb);\n}\n')
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"),
                           str(src)])


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    dims = (C.c_size_t * 2)(64, 64)
    ebs, pts, rng = (C.c_double * 1)(1e-3), (H.RdPoint * 1)(), (C.c_double * 2)(-7.0, -7.0)
    info, eb, ps = H.CompressInfo(), C.c_double(-7.0), C.c_double(-7.0)
    assert lib.dctzhip_rd_probe_nd(None, None, 2, dims, 1, 1, ebs, pts, rng) == H.E_ARG
    assert lib.dctzhip_compress_psnr_nd(None, None, 2, dims, 1, 60.0, None, None, None, C.byref(info), C.byref(eb), C.byref(ps)) == H.E_ARG
    assert rng[0] == -7.0 and eb.value == -7.0 and ps.value == -7.0


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_compress_psnr_nd_refuses_before_it_asks_for_a_device(so):
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    ps = C.POINTER(C.c_size_t)
    lib.dctz_compress_psnr_nd.restype = C.c_int
    lib.dctz_compress_psnr_nd.argtypes = [C.POINTER(TVar), C.c_int, ps, ps, C.POINTER(TVar), C.c_double, C.POINTER(C.c_double)]
    lib.dctz_compress_psnr.restype = C.c_int
    lib.dctz_compress_psnr.argtypes = [C.POINTER(TVar), C.c_int, ps, C.POINTER(TVar), C.c_double, C.POINTER(C.c_double)]
    lib.dctz_set_block_dims.restype = C.c_int
    lib.dctz_set_block_dims.argtypes = [C.c_int, ps]
    x0 = np.linspace(0.0, 1.0, 64 * 64).reshape(64, 64)
    x = x0.copy()
    v = TVar()
    v.datatype = 1
    v.buf.d = x.ctypes.data_as(C.POINTER(C.c_double))
    z = np.full(4096, 0x5A, np.uint8)
    vz = TVar()
    vz.datatype = 1
    vz.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    size, eb = C.c_size_t(12345), C.c_double(-7.0)
    arr = lambda *d: (C.c_size_t * len(d))(*d)

    def call(var=C.byref(v), nd=2, dims=arr(64, 64), out=C.byref(size), var_z=C.byref(vz), target=60.0, used=C.byref(eb)):
        return lib.dctz_compress_psnr_nd(var, nd, dims, out, var_z, target, used)

    if "qt" in so:
        assert call() == -1                                  # always, whatever the arguments
    # the pointers, the type, the target
    assert call(var=None) == -1 and call(out=None) == -1 and call(var_z=None) == -1 and call(used=None) == -1
    bad = TVar()
    bad.datatype = 7
    bad.buf.d = v.buf.d
    assert call(var=C.byref(bad)) == -1
    assert call(target=float("nan")) == -1 and call(target=float("inf")) == -1
    # the shape: ndims, NULL, an extent of 0 or beyond an int, a product or a tile count beyond an int
    for kw in (dict(nd=1, dims=arr(4096)), dict(nd=0), dict(nd=4, dims=arr(8, 8, 8, 8)), dict(dims=None), dict(dims=arr(0, 64)),
               dict(dims=arr(64, 0)), dict(dims=arr(2 ** 31, 2)), dict(dims=arr(2 ** 16, 2 ** 15)), dict(nd=3, dims=arr(2 ** 11, 2 ** 10, 2 ** 10)),
               dict(nd=3, dims=arr(64, 64, 0)), dict(dims=arr(1, 2 ** 30))):
        assert call(**kw) == -1, kw
    # a pending request of the caller's: refused, and the request stays pending -- the flat call still sees it
    assert lib.dctz_set_block_dims(2, arr(32, 128)) == 0
    assert call() == -1
    assert lib.dctz_compress_psnr(C.byref(v), 4096, C.byref(size), C.byref(vz), 60.0, C.byref(eb)) == -1
    assert lib.dctz_set_block_dims(0, None) == 0
    assert size.value == 12345 and eb.value == -7.0 and np.array_equal(x, x0) and (z == 0x5A).all()
