"""The drop-in calls of the tiled missing-value layer (include/dctz.h: dctz_compress_masked_nd / dctz_decompress_masked_nd, both
builds): the container is byte for byte dctz_set_block_dims + dctz_compress of the numpy-filled host array and the caller's
buffer is left as that call leaves it; the "DZMK" blob carries the header fields with n = prod dims and a payload that
Python's zlib inflates to the mask words of the array in C order; decompress writes the fill into the missing elements, with
and without a correction blob built by dctz_fixup_build against the filled array (the composed guarantee)."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import mask_cases as M
from tests import ndmask_cases as N

pytestmark = pytest.mark.gpu

EB = 1e-3
FILL = -9.96921e36
SHAPES = ((61, 93), (13, 30, 45))                 # ragged in every axis: edge tiles, the element path, the atomic mask path


class DMissing(C.Structure):
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


def _lib(mode):
    lib = D._lib(mode)
    ps = C.POINTER(C.c_size_t)
    lib.dctz_compress_masked_nd.restype = C.c_int
    lib.dctz_compress_masked_nd.argtypes = [C.POINTER(D.TVar), C.c_int, ps, ps, C.POINTER(D.TVar), C.c_double, C.POINTER(DMissing),
                                            C.c_double, C.POINTER(C.c_void_p), ps]
    lib.dctz_decompress_masked_nd.restype = C.c_int
    lib.dctz_decompress_masked_nd.argtypes = [C.POINTER(D.TVar), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(D.TVar)]
    lib.dctz_fixup_build.restype = C.c_int
    lib.dctz_fixup_build.argtypes = [C.POINTER(D.TVar), C.POINTER(D.TVar), C.c_int, C.c_double, C.POINTER(C.c_void_p), ps]
    return lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _holey(shape, dtype):
    x = (N.field(shape, dtype) * dtype(5.5)).astype(dtype)        # sf = 10: the in-place division shows
    miss = N.blobs(shape) | N.pattern("random30", shape) | N.pattern("edge_tile_all", shape) | N.pattern("tile_last_only", shape)
    assert 0.3 < miss.mean() < 0.7
    x[miss] = 1e36
    return x, miss


def _zvar(z, dtype):
    return D._tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["2-D", "3-D"])
def test_round_trip(mode, dtype, shape):
    lib = _lib(mode)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    x, miss = _holey(shape, dtype)
    n, nd = x.size, len(shape)
    dims = (C.c_size_t * nd)(*shape)
    filled = N.fill(x, miss)
    # the reference: dctz_set_block_dims + dctz_compress of the filled host array
    ref_in = filled.copy()
    zref = np.zeros(2 * n * x.itemsize + (1 << 16), np.uint8)
    szref = C.c_size_t(0)
    assert lib.dctz_set_block_dims(nd, dims) == 0
    assert lib.dctz_compress(C.byref(D._tvar(ref_in.reshape(-1))), n, C.byref(szref), C.byref(_zvar(zref, dtype)), EB) == 1
    full = np.empty(shape, dtype)
    assert lib.dctz_decompress(C.byref(_zvar(zref, dtype)), C.byref(D._tvar(full.reshape(-1)))) == 1
    # the masked call
    buf = x.copy()
    z = np.zeros_like(zref)
    sz, blob, nbytes = C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
    rule = DMissing(M.MISS_VALUE, 1e36, 0.0)
    assert lib.dctz_compress_masked_nd(C.byref(D._tvar(buf.reshape(-1))), nd, dims, C.byref(sz), C.byref(_zvar(z, dtype)), EB, C.byref(rule),
                                       FILL, C.byref(blob), C.byref(nbytes)) == 1
    fix = C.c_void_p()
    try:
        assert sz.value == szref.value and np.array_equal(z[:sz.value], zref[:sz.value]), "the container is that pair's"
        assert np.array_equal(_bits(buf), _bits(ref_in)), "var->buf: filled and divided by sf"
        assert not np.array_equal(_bits(ref_in), _bits(filled))
        raw = C.string_at(blob, nbytes.value)
        magic, version, dt, flags, hn, count, fill, words, payload = struct.unpack("<4sIIIQQdII", raw[:48])
        assert (magic, version, dt, flags) == (b"DZMK", 1, 1 if dtype == np.float64 else 0, M.MISS_VALUE)
        assert (hn, count, fill, words, payload) == (n, int(miss.sum()), FILL, -(-n // 64), len(raw) - 48)
        d = zlib.decompressobj()
        w = np.frombuffer(d.decompress(raw[48:]), dtype=np.uint64)
        assert d.eof and d.unused_data == b""                        # one stream, nothing behind it
        assert np.array_equal(w, N.mask_words(miss))
        # the next plain call is flat again: the request the masked call made for itself was consumed by it
        flat_in = filled.copy().reshape(-1)
        zf = np.zeros_like(zref)
        szf = C.c_size_t(0)
        assert lib.dctz_compress(C.byref(D._tvar(flat_in)), n, C.byref(szf), C.byref(_zvar(zf, dtype)), EB) == 1
        assert (int(zf[:4].view(np.uint32)[0]) >> 8) & 0xFF == 0 and (int(z[:4].view(np.uint32)[0]) >> 8) & 0xFF == nd
        # decode: the fill where the mask says so, the plain decode elsewhere
        out = np.empty(shape, dtype)
        assert lib.dctz_decompress_masked_nd(C.byref(_zvar(z, dtype)), blob, nbytes.value, None, 0, C.byref(D._tvar(out.reshape(-1)))) == 1
        assert np.array_equal(_bits(out), _bits(np.where(miss, dtype(FILL), full)))
        # with a correction list built against the FILLED array: the composed guarantee
        bound = 0.1 * EB * 10.0                   # (well inside the quantisation error of either geometry: the list is not empty)
        fbytes = C.c_size_t(0)
        ref = filled.copy()
        assert lib.dctz_fixup_build(C.byref(_zvar(z, dtype)), C.byref(D._tvar(ref.reshape(-1))), n, bound, C.byref(fix), C.byref(fbytes)) == 1
        version, listed = struct.unpack("<I", C.string_at(fix, 8)[4:8])[0], int(np.frombuffer(C.string_at(fix, 48)[32:40], dtype=np.uint64)[0])
        with np.errstate(invalid="ignore"):
            far = ~(np.abs(filled - full) <= dtype(bound))
        assert version == 2 and listed == int(far.sum()) > 0
        out2 = np.empty(shape, dtype)
        assert lib.dctz_decompress_masked_nd(C.byref(_zvar(z, dtype)), blob, nbytes.value, fix, fbytes.value, C.byref(D._tvar(out2.reshape(-1)))) == 1
        assert np.array_equal(_bits(out2), _bits(np.where(miss, dtype(FILL), np.where(far, filled, full))))
        same = _bits(out2) == _bits(x)
        with np.errstate(invalid="ignore", over="ignore"):
            near = np.abs(x - out2) <= dtype(bound)
        assert bool((same | near)[~miss].all()) and bool((_bits(out2)[miss] == _bits(np.array([FILL], dtype))[0]).all())
        # refusals on a real container: a blob of the streams' positions instead of the elements, a cut one, a cut correction blob
        sent = np.full(n, 7.0, dtype)
        for what, b in (("cut", raw[:-3]), ("n", raw[:16] + struct.pack("<Q", n + 64) + raw[24:]), ("payload", raw[:48] + bytes(len(raw) - 48))):
            bb = C.create_string_buffer(b, len(b))
            assert lib.dctz_decompress_masked_nd(C.byref(_zvar(z, dtype)), bb, len(b), None, 0, C.byref(D._tvar(sent))) == -1, what
        assert lib.dctz_decompress_masked_nd(C.byref(_zvar(z, dtype)), blob, nbytes.value, fix, fbytes.value - 8, C.byref(D._tvar(sent))) == -1
        assert lib.dctz_decompress_masked_nd(C.byref(_zvar(zf, dtype)), blob, nbytes.value, None, 0, C.byref(D._tvar(sent))) == -1, "flat container"
        assert (sent == 7.0).all()
    finally:
        libc.free(blob)
        libc.free(fix)
