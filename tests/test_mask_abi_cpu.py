"""CPU-side checks of the missing-value layer: dctzhip_mask_words, dctzhip_mask_build, dctzhip_mask_apply and
dctzhip_compress_masked are exported by libdctzhip.so with the documented argument types, dctz_compress_masked and
dctz_decompress_masked by both drop-in libraries (which link the first); the prototypes stand in the headers; the device ABI
refuses a NULL context before it touches a GPU (the other pre-launch refusals need a context, which needs a device:
tests/test_gpu_mask.py makes them); the drop-in refuses a rule or a blob that does not fit before anything else."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
CALLS = ("dctzhip_mask_words", "dctzhip_mask_build", "dctzhip_mask_apply", "dctzhip_compress_masked")
DROPIN = ("dctz_compress_masked", "dctz_decompress_masked")


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
    for name in ("mask_build", "mask_apply", "compress_masked"):
        assert hasattr(H.Context, name)
    assert (H.MISS_NAN, H.MISS_INF, H.MISS_VALUE, H.MISS_ABS_GE) == (1, 2, 4, 8)


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_calls(so):
    assert set(DROPIN) <= _exported(so)
    # the device calls reach a drop-in's user through the library it links
    needed = subprocess.check_output(["readelf", "-d", os.path.join(LIB, so)], text=True)
    assert "libdctzhip.so" in needed


def test_argument_types_and_prototypes(tmp_path):
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    vp, ps = C.c_void_p, C.POINTER(C.c_size_t)
    assert lib.dctzhip_mask_words.restype is C.c_size_t and lib.dctzhip_mask_words.argtypes == [C.c_size_t]
    assert lib.dctzhip_mask_build.restype is C.c_int
    assert lib.dctzhip_mask_build.argtypes == [vp, vp, C.c_size_t, C.c_int, C.POINTER(H.Missing), vp, vp, C.POINTER(C.c_uint64)]
    assert lib.dctzhip_mask_apply.restype is C.c_int
    assert lib.dctzhip_mask_apply.argtypes == [vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_int, ps, ps, ps, vp]
    assert lib.dctzhip_compress_masked.restype is C.c_int
    assert lib.dctzhip_compress_masked.argtypes == [vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_int, C.POINTER(H.Missing), vp, vp, vp, vp, vp,
                                                    C.POINTER(H.CompressInfo), C.POINTER(C.c_uint64)]
    hdr = _header("dctz_hip.h")
    assert "size_t dctzhip_mask_words(size_t n);" in hdr
    assert "typedef struct { unsigned flags; double value; double limit; } dctzhip_missing;" in hdr
    assert ("int dctzhip_mask_build(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, const dctzhip_missing *miss, "
            "uint64_t *d_mask, void *d_filled /* NULL, == d_in, or disjoint */, uint64_t *count /* host */);") in hdr
    assert ("int dctzhip_mask_apply(dctzhip_ctx *ctx, const uint64_t *d_mask, size_t n, int dtype, double fill, int ndim, "
            "const size_t *dims, const size_t *lo, const size_t *hi, void *d_out);") in hdr
    assert ("int dctzhip_compress_masked(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, double error_bound, int mode, "
            "const dctzhip_missing *miss, void *d_bin_index, float *d_dc, float *d_ac_exact, uint64_t *d_mask, "
            "void *d_filled /* or NULL: context scratch, kept */, dctzhip_cinfo *info, uint64_t *count /* host */);") in hdr
    hdr = _header("dctz.h")
    assert "typedef struct { unsigned flags; double value; double limit; } dctz_missing;" in hdr
    assert ("int dctz_compress_masked(t_var *var, int N, size_t *outSize, t_var *var_z, double error_bound, const dctz_missing *miss, "
            "double fill, void **mask_blob, size_t *mask_bytes);") in hdr
    assert ("int dctz_decompress_masked(t_var *var_z, const void *mask_blob, size_t mask_bytes, const void *fix_blob /* or NULL */, "
            "size_t fix_bytes, t_var *var_r);") in hdr
    # the C compiler and the binding agree on the flags and on the rule's layout
    src = tmp_path / "miss.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dctz_hip.h"\nint main(void) { printf("%u %u %u %u %zu %zu %zu\\n", '
                   'DCTZHIP_MISS_NAN, DCTZHIP_MISS_INF, DCTZHIP_MISS_VALUE, DCTZHIP_MISS_ABS_GE, sizeof(dctzhip_missing), '
                   'offsetof(dctzhip_missing, value), offsetof(dctzhip_missing, limit)); return 0; }\n')
    exe = tmp_path / "miss"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [1, 2, 4, 8, C.sizeof(H.Missing), H.Missing.value.offset, H.Missing.limit.offset]


def test_mask_words_values():
    import dctz_amd
    lib = dctz_amd.load_library()
    for n, want in ((1, 1), (63, 1), (64, 1), (65, 2), (4096, 64), (4097, 65), (2 ** 31 - 1, 2 ** 25)):
        assert lib.dctzhip_mask_words(n) == want == -(-n // 64), n


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    count = C.c_uint64(0)
    one, zero = (C.c_size_t * 1)(4096), (C.c_size_t * 1)(0)
    miss = H.Missing(H.MISS_NAN, 0.0, 0.0)
    info = H.CompressInfo()
    assert lib.dctzhip_mask_build(None, None, 4096, 1, C.byref(miss), None, None, C.byref(count)) == H.E_ARG
    assert lib.dctzhip_mask_apply(None, None, 4096, 1, 0.0, 1, one, zero, one, None) == H.E_ARG
    assert lib.dctzhip_compress_masked(None, None, 4096, 1, 1e-3, 0, C.byref(miss), None, None, None, None, None, C.byref(info),
                                       C.byref(count)) == H.E_ARG


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


class DMissing(C.Structure):
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


def _blob(n, is_d, count=0, magic=b"DZMK", version=1, dtype=None, flags=4, fill=1e36, words=None, payload=None, claim=None):
    w = -(-n // 64) if words is None else words
    z = zlib.compress(bytes(8 * (-(-n // 64))), 6) if payload is None else payload
    head = magic + struct.pack("<IIIQQdII", version, int(is_d) if dtype is None else dtype, flags, n, count, fill, w,
                               len(z) if claim is None else claim)
    assert len(head) == 48
    return head + z


def _container(n):
    """56 header bytes of a flat fp64 container of n elements (dctz.h: struct header), nothing behind them that could be read."""
    z = np.zeros(64, np.uint8)
    z[0:4] = np.frombuffer(struct.pack("<I", 1), np.uint8)            # datatype DOUBLE, flat blocks
    z[4:8] = np.frombuffer(struct.pack("<I", n), np.uint8)            # num_elements
    zv = TVar()
    zv.datatype = 1
    zv.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    return z, zv


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_a_blob_that_does_not_fit_the_container_is_refused_first(so):
    """-1 from the headers and the payload alone: no section is inflated and no device is asked for (there is none here; a call
    that went on would end the process)."""
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    lib.dctz_decompress_masked.restype = C.c_int
    lib.dctz_decompress_masked.argtypes = [C.POINTER(TVar), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(TVar)]
    n = 3 * 4096 + 37
    z, zv = _container(n)
    out = np.zeros(n, np.float64)
    ov = TVar()
    ov.datatype = 1
    ov.buf.d = out.ctypes.data_as(C.POINTER(C.c_double))
    good = _blob(n, True, count=5)
    words = -(-n // 64)
    bad = {"magic": _blob(n, True, 5, magic=b"DZMJ"), "version": _blob(n, True, 5, version=2), "dtype": _blob(n, True, 5, dtype=0),
           "n": _blob(n + 1, True, 5), "count": _blob(n, True, n + 1), "words": _blob(n, True, 5, words=words + 1),
           "no flags": _blob(n, True, 5, flags=0), "unknown flags": _blob(n, True, 5, flags=16),
           "short": good[:-1], "long": good + bytes(1), "header cut": good[:40], "header only": good[:48],
           "claims less": _blob(n, True, 5, claim=len(good) - 49), "empty payload": _blob(n, True, 5, payload=b""),
           # payloads that are sound zlib streams of the wrong length, and one that is no zlib stream
           "inflates short": _blob(n, True, 5, payload=zlib.compress(bytes(8 * words - 8), 6)),
           "inflates long": _blob(n, True, 5, payload=zlib.compress(bytes(8 * words + 8), 6)),
           "inflates one byte long": _blob(n, True, 5, payload=zlib.compress(bytes(8 * words + 1), 6)),
           "damaged": good[:48] + bytes(len(good) - 48)}
    for what, b in bad.items():
        buf = C.create_string_buffer(b, len(b))
        assert lib.dctz_decompress_masked(C.byref(zv), buf, len(b), None, 0, C.byref(ov)) == -1, what
    assert lib.dctz_decompress_masked(C.byref(zv), None, 0, None, 0, C.byref(ov)) == -1
    gbuf = C.create_string_buffer(good, len(good))
    # a correction blob that does not fit is refused with a mask blob that does
    fx = b"DZFX" + struct.pack("<IIIQQQd", 1, 1, 0, n + 1, 4, 0, 0.1) + bytes(24)
    fbuf = C.create_string_buffer(fx, len(fx))
    assert lib.dctz_decompress_masked(C.byref(zv), gbuf, len(good), fbuf, len(fx), C.byref(ov)) == -1
    assert lib.dctz_decompress_masked(C.byref(zv), gbuf, len(good), gbuf, len(good), C.byref(ov)) == -1
    # a DZND container is out of scope whatever the blob says
    z[0:4] = np.frombuffer(struct.pack("<I", 1 | (2 << 8)), np.uint8)
    assert lib.dctz_decompress_masked(C.byref(zv), gbuf, len(good), None, 0, C.byref(ov)) == -1
    assert not out.any()


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_compress_masked_refuses_before_it_asks_for_a_device(so):
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    lib.dctz_compress_masked.restype = C.c_int
    lib.dctz_compress_masked.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(TVar), C.c_double, C.POINTER(DMissing),
                                         C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.dctz_set_block_dims.restype = C.c_int
    lib.dctz_set_block_dims.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    n = 4096
    x = np.ones(n, np.float64)
    v = TVar()
    v.datatype = 1
    v.buf.d = x.ctypes.data_as(C.POINTER(C.c_double))
    vz = TVar()
    size, blob, nbytes = C.c_size_t(0), C.c_void_p(None), C.c_size_t(0)

    def call(miss, var=C.byref(v), N=n):
        return lib.dctz_compress_masked(var, N, C.byref(size), C.byref(vz), 1e-3, C.byref(miss) if miss is not None else None, 0.0,
                                        C.byref(blob), C.byref(nbytes))

    for miss in (None, DMissing(0, 0, 0), DMissing(16, 0, 0), DMissing(4, float("nan"), 0), DMissing(8, 0, 0.0), DMissing(8, 0, -2.0),
                 DMissing(8, 0, float("inf")), DMissing(8, 0, float("nan"))):
        assert call(miss) == -1
    assert call(DMissing(1, 0, 0), N=0) == -1 and call(DMissing(1, 0, 0), var=None) == -1
    # pending block dimensions: flat blocks only (the dimensions stay pending for the call they were meant for)
    dims = (C.c_size_t * 2)(64, 64)
    assert lib.dctz_set_block_dims(2, dims) == 0
    assert call(DMissing(1, 0, 0)) == -1
    assert lib.dctz_set_block_dims(0, None) == 0
    assert call(None) == -1
    assert blob.value is None and nbytes.value == 0 and np.array_equal(x, np.ones(n))


def test_the_blob_layout_is_written_down_once():
    """csrc/dctz_mask_blob.h holds the layout; the library includes it and spells no offset of its own."""
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "dctz_mask_blob.h")) as f:
        hdr = f.read()
    assert '#define DZMK_MAGIC "DZMK"' in hdr and "#define DZMK_HEADER_BYTES 48" in hdr and "#define DZMK_ZLIB_LEVEL 6" in hdr
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "libdctz.c")) as f:
        src = f.read()
    assert '#include "dctz_mask_blob.h"' in src and '"DZMK"' not in re.sub(r"/\*.*?\*/", "", src, flags=re.S)
