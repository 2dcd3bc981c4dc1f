"""CPU-side checks of the tiled missing-value layer: dctzhip_mask_build_nd and dctzhip_compress_masked_nd are exported by
libdctzhip.so with the documented argument types, dctz_compress_masked_nd and dctz_decompress_masked_nd by both drop-in
libraries; the prototypes stand in the headers and compile; the device ABI refuses a NULL context before it touches a GPU (the
other pre-launch refusals need a context: tests/test_gpu_ndmask.py makes them); the drop-in refuses a rule, a shape, a pending
request, a container or a blob that does not fit before it asks for a device (there is none here: a call that went on would
end the process)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
CALLS = ("dctzhip_mask_build_nd", "dctzhip_compress_masked_nd")
DROPIN = ("dctz_compress_masked_nd", "dctz_decompress_masked_nd")


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
    for name in ("mask_build_nd", "compress_masked_nd"):
        assert hasattr(H.Context, name)


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_calls(so):
    assert set(DROPIN) <= _exported(so)


def test_argument_types_and_prototypes(tmp_path):
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    vp, ps = C.c_void_p, C.POINTER(C.c_size_t)
    assert lib.dctzhip_mask_build_nd.restype is C.c_int
    assert lib.dctzhip_mask_build_nd.argtypes == [vp, vp, C.c_int, ps, C.c_int, C.POINTER(H.Missing), vp, vp, C.POINTER(C.c_uint64)]
    assert lib.dctzhip_compress_masked_nd.restype is C.c_int
    assert lib.dctzhip_compress_masked_nd.argtypes == [vp, vp, C.c_int, ps, C.c_int, C.c_double, C.c_int, C.POINTER(H.Missing), vp, vp, vp,
                                                       vp, vp, C.POINTER(H.CompressInfo), C.POINTER(C.c_uint64)]
    hdr = _header("dctz_hip.h")
    assert ("int dctzhip_mask_build_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype, "
            "const dctzhip_missing *miss, uint64_t *d_mask, void *d_filled /* NULL, == d_in, or disjoint */, "
            "uint64_t *count /* host */);") in hdr
    assert ("int dctzhip_compress_masked_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype, "
            "double error_bound, int mode, const dctzhip_missing *miss, void *d_bin_index, float *d_dc, float *d_ac_exact, "
            "uint64_t *d_mask, void *d_filled /* or NULL: context scratch, kept */, dctzhip_cinfo *info, "
            "uint64_t *count /* host */);") in hdr
    hdr = _header("dctz.h")
    assert ("int dctz_compress_masked_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, double error_bound, "
            "const dctz_missing *miss, double fill, void **mask_blob, size_t *mask_bytes);") in hdr
    assert ("int dctz_decompress_masked_nd(t_var *var_z, const void *mask_blob, size_t mask_bytes, const void *fix_blob /* or NULL */, "
            "size_t fix_bytes, t_var *var_r);") in hdr
    # the prototypes compile, and calls written after the issue's signatures compile against them without a warning
    src = tmp_path / "proto.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "dctz_hip.h"\n#include "dctz.h"\n'
                   'int use(dctzhip_ctx *c, void *p, const size_t *dims, const dctzhip_missing *m, uint64_t *mask, dctzhip_cinfo *info,\n'
                   '        uint64_t *cnt, t_var *v, size_t *sz, const dctz_missing *dm, void **blob) {\n'
                   '  int (*a)(dctzhip_ctx *, const void *, int, const size_t *, int, const dctzhip_missing *, uint64_t *, void *, uint64_t *) = dctzhip_mask_build_nd;\n'
                   '  int (*b)(t_var *, const void *, size_t, const void *, size_t, t_var *) = dctz_decompress_masked_nd;\n'
                   '  return a(c, p, 2, dims, DCTZHIP_F64, m, mask, NULL, cnt)\n'
                   '       + dctzhip_compress_masked_nd(c, p, 3, dims, DCTZHIP_F32, 1e-3, DCTZHIP_QT, m, p, (float *)p, (float *)p, mask, NULL, info, cnt)\n'
                   '       + dctz_compress_masked_nd(v, 2, dims, sz, v, 1e-3, dm, 0.0, blob, sz) + b(v, *blob, *sz, NULL, 0, v);\n}\n')
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"),
                           str(src)])


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    count = C.c_uint64(7)
    dims = (C.c_size_t * 2)(64, 64)
    miss = H.Missing(H.MISS_NAN, 0.0, 0.0)
    info = H.CompressInfo()
    assert lib.dctzhip_mask_build_nd(None, None, 2, dims, 1, C.byref(miss), None, None, C.byref(count)) == H.E_ARG
    assert lib.dctzhip_compress_masked_nd(None, None, 2, dims, 1, 1e-3, 0, C.byref(miss), None, None, None, None, None, C.byref(info),
                                          C.byref(count)) == H.E_ARG
    assert count.value == 7


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


class DMissing(C.Structure):
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_compress_masked_nd_refuses_before_it_asks_for_a_device(so):
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    ps = C.POINTER(C.c_size_t)
    lib.dctz_compress_masked_nd.restype = C.c_int
    lib.dctz_compress_masked_nd.argtypes = [C.POINTER(TVar), C.c_int, ps, ps, C.POINTER(TVar), C.c_double, C.POINTER(DMissing), C.c_double,
                                            C.POINTER(C.c_void_p), ps]
    lib.dctz_compress_masked.restype = C.c_int
    lib.dctz_compress_masked.argtypes = [C.POINTER(TVar), C.c_int, ps, C.POINTER(TVar), C.c_double, C.POINTER(DMissing), C.c_double,
                                         C.POINTER(C.c_void_p), ps]
    lib.dctz_set_block_dims.restype = C.c_int
    lib.dctz_set_block_dims.argtypes = [C.c_int, ps]
    x = np.ones((64, 64), np.float64)
    v = TVar()
    v.datatype = 1
    v.buf.d = x.ctypes.data_as(C.POINTER(C.c_double))
    vz = TVar()
    size, blob, nbytes = C.c_size_t(0), C.c_void_p(None), C.c_size_t(0)
    arr = lambda *d: (C.c_size_t * len(d))(*d)
    good = DMissing(1, 0, 0)

    def call(miss=good, var=C.byref(v), nd=2, dims=arr(64, 64)):
        blob.value = 0x1234                                       # (a refusal leaves NULL behind, whatever stood there)
        rc = lib.dctz_compress_masked_nd(var, nd, dims, C.byref(size), C.byref(vz), 1e-3, C.byref(miss) if miss is not None else None, 0.0,
                                         C.byref(blob), C.byref(nbytes))
        assert blob.value is None
        return rc

    # the rule
    for miss in (None, DMissing(0, 0, 0), DMissing(16, 0, 0), DMissing(4, float("nan"), 0), DMissing(8, 0, 0.0), DMissing(8, 0, -2.0),
                 DMissing(8, 0, float("inf")), DMissing(8, 0, float("nan"))):
        assert call(miss=miss) == -1
    assert call(var=None) == -1
    # the shape: ndims, NULL, an extent of 0 or beyond an int, a product beyond an int
    for kw in (dict(nd=1, dims=arr(4096)), dict(nd=0), dict(nd=4, dims=arr(8, 8, 8, 8)), dict(dims=None), dict(dims=arr(0, 64)),
               dict(dims=arr(64, 0)), dict(dims=arr(2 ** 31, 2)), dict(dims=arr(2 ** 16, 2 ** 15)), dict(nd=3, dims=arr(2 ** 11, 2 ** 10, 2 ** 10)),
               dict(nd=3, dims=arr(64, 64, 0))):
        assert call(**kw) == -1, kw
    # a pending request of the caller's: refused, and the request stays pending -- the flat call still sees it
    assert lib.dctz_set_block_dims(2, arr(32, 128)) == 0
    assert call() == -1
    assert lib.dctz_compress_masked(C.byref(v), 4096, C.byref(size), C.byref(vz), 1e-3, C.byref(good), 0.0, C.byref(blob), C.byref(nbytes)) == -1
    assert lib.dctz_set_block_dims(0, None) == 0
    assert call(miss=None) == -1
    assert nbytes.value == 0 and size.value == 0 and np.array_equal(x, np.ones((64, 64)))


def _mask_blob(n, is_d, count=0, version=1, payload=None):
    words = -(-n // 64)
    z = zlib.compress(bytes(8 * words), 6) if payload is None else payload
    head = b"DZMK" + struct.pack("<IIIQQdII", version, int(is_d), 4, n, count, 1e36, words, len(z))
    assert len(head) == 48
    return head + z


def _fix_blob_nd(is_d, dims, n, nblk):
    """A tiled (version-2) correction blob without entries: 72 header bytes, the tile starts."""
    tiles = -(-nblk * 64 // 4096)
    d = list(dims) + [0] * (3 - len(dims))
    head = b"DZFX" + struct.pack("<IIIQQQd", 2, int(is_d), len(dims), n, tiles, 0, 0.1) + struct.pack("<QQQ", *d)
    assert len(head) == 72
    return head + bytes((4 * (tiles + 1) + 7) // 8 * 8)


def _container(so, dims, n=None, nd=None):
    """The header bytes of an fp64 DZND container with empty sections (dctz.h: struct header; the extents sit behind the sections,
    in a QT build behind the table), nothing behind them that could be inflated."""
    at = 56 + (64 * 8 if "qt" in so else 0)
    z = np.zeros(at + 16 + 64, np.uint8)
    nd = len(dims) if nd is None else nd
    z[0:4] = np.frombuffer(struct.pack("<I", 1 | (nd << 8)), np.uint8)             # datatype DOUBLE + geometry
    z[4:8] = np.frombuffer(struct.pack("<I", int(np.prod(dims)) if n is None else n), np.uint8)
    z[at:at + 16] = np.frombuffer(b"DZND" + struct.pack("<III", *(list(dims) + [1] * (3 - len(dims)))), np.uint8)
    zv = TVar()
    zv.datatype = 1
    zv.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    return z, zv


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_decompress_masked_nd_refuses_what_does_not_fit_first(so):
    """-1 from the headers and the payload alone, and nothing written to the output."""
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    lib.dctz_decompress_masked_nd.restype = C.c_int
    lib.dctz_decompress_masked_nd.argtypes = [C.POINTER(TVar), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(TVar)]
    dims = (40, 100)
    n, nblk = 4000, 5 * 13
    out = np.zeros(n, np.float64)
    ov = TVar()
    ov.datatype = 1
    ov.buf.d = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(zv, mask, fix=None, var_r=C.byref(ov)):
        mb = C.create_string_buffer(mask, len(mask)) if mask is not None else None
        fb = C.create_string_buffer(fix, len(fix)) if fix is not None else None
        return lib.dctz_decompress_masked_nd(C.byref(zv) if zv is not None else None, mb, len(mask) if mask is not None else 0, fb,
                                             len(fix) if fix is not None else 0, var_r)

    good, words = _mask_blob(n, True, 5), -(-n // 64)
    z, zv = _container(so, dims)
    # a flat container, whatever the blob says
    zf, zfv = _container(so, dims, nd=0)
    assert call(zfv, good) == -1
    # a tiled container whose extents are none or do not multiply to its n
    zb, zbv = _container(so, dims, n=n + 1)
    assert call(zbv, _mask_blob(n + 1, True)) == -1 and call(zbv, good) == -1
    z0, z0v = _container(so, (40, 0), n=n)
    assert call(z0v, good) == -1
    # a mask blob whose n is not the product of the extents (the streams' 64 nblk positions are not it either)
    for what, b in {"n + 1": _mask_blob(n + 1, True), "positions": _mask_blob(64 * nblk, True), "fp32": _mask_blob(n, False),
                    "version": _mask_blob(n, True, version=2), "count": _mask_blob(n, True, n + 1), "short": good[:-1], "long": good + bytes(1),
                    "header only": good[:48], "inflates short": _mask_blob(n, True, payload=zlib.compress(bytes(8 * words - 8), 6)),
                    "inflates long": _mask_blob(n, True, payload=zlib.compress(bytes(8 * words + 1), 6)),
                    "damaged": good[:48] + bytes(len(good) - 48)}.items():
        assert call(zv, b) == -1, what
    assert call(zv, None) == -1 and call(None, good) == -1 and call(zv, good, var_r=None) == -1
    # a correction blob: the flat kind (version 1), the tiled kind with other extents, and the mask blob in its place
    flat = b"DZFX" + struct.pack("<IIIQQQd", 1, 1, 0, n, 1, 0, 0.1) + bytes(8)
    assert call(zv, good, fix=flat) == -1
    assert call(zv, good, fix=_fix_blob_nd(True, (100, 40), n, nblk)) == -1
    assert call(zv, good, fix=_fix_blob_nd(False, dims, n, nblk)) == -1
    assert call(zv, good, fix=good) == -1
    # ... and a sound tiled correction blob does not save a mask blob that does not fit
    assert call(zv, _mask_blob(n + 1, True), fix=_fix_blob_nd(True, dims, n, nblk)) == -1
    assert not out.any()
