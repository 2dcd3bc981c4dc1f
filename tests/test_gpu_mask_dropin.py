"""The drop-in calls of the missing-value layer (include/dctz.h: dctz_compress_masked / dctz_decompress_masked, both builds):
the container is byte for byte dctz_compress of the filled host array and the caller's buffer is left as that call leaves
it; the "DZMK" blob (csrc/dctz_mask_blob.h) carries the header fields and a payload that Python's zlib inflates to the mask
words; decompress writes the fill into the missing elements, with and without a correction blob; each refusal returns -1."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import mask_cases as M
from tests import workloads as W

pytestmark = pytest.mark.gpu

EB = 1e-3
N = 3 * 4096 + 5 * 64 + 37
FILL = -9.96921e36


class DMissing(C.Structure):
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


def _lib(mode):
    lib = D._lib(mode)
    lib.dctz_compress_masked.restype = C.c_int
    lib.dctz_compress_masked.argtypes = [C.POINTER(D.TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(D.TVar), C.c_double, C.POINTER(DMissing),
                                         C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.dctz_decompress_masked.restype = C.c_int
    lib.dctz_decompress_masked.argtypes = [C.POINTER(D.TVar), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(D.TVar)]
    lib.dctz_fixup_build.restype = C.c_int
    lib.dctz_fixup_build.argtypes = [C.POINTER(D.TVar), C.POINTER(D.TVar), C.c_int, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    return lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _holey(dtype):
    x = W.ragged(N, dtype, scale=37.0)                    # sf = 10: the in-place division shows
    miss = M.pattern("random30", N) | M.pattern("across_boundaries", N) | M.pattern("last_block_leading", N) | M.pattern("whole_block", N)
    x[miss] = 1e36
    return x, miss


def _zvar(z, dtype):
    return D._tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_round_trip(mode, dtype):
    lib = _lib(mode)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    x, miss = _holey(dtype)
    filled = M.fill(x, miss)
    # the reference: dctz_compress of the filled host array
    ref_in = filled.copy()
    zref = np.zeros(N * x.itemsize + (1 << 16), np.uint8)
    szref = C.c_size_t(0)
    assert lib.dctz_compress(C.byref(D._tvar(ref_in)), N, C.byref(szref), C.byref(_zvar(zref, dtype)), EB) == 1
    full = np.empty_like(x)
    assert lib.dctz_decompress(C.byref(_zvar(zref, dtype)), C.byref(D._tvar(full))) == 1
    # the masked call
    buf = x.copy()
    z = np.zeros_like(zref)
    sz, blob, nbytes = C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
    rule = DMissing(M.MISS_VALUE, 1e36, 0.0)
    assert lib.dctz_compress_masked(C.byref(D._tvar(buf)), N, C.byref(sz), C.byref(_zvar(z, dtype)), EB, C.byref(rule), FILL,
                                    C.byref(blob), C.byref(nbytes)) == 1
    fix = C.c_void_p()
    try:
        assert sz.value == szref.value and np.array_equal(z[:sz.value], zref[:sz.value]), "the container is dctz_compress(filled)'s"
        assert np.array_equal(_bits(buf), _bits(ref_in)), "var->buf: filled and divided by sf"
        assert not np.array_equal(_bits(ref_in), _bits(filled))
        raw = C.string_at(blob, nbytes.value)
        magic, version, dt, flags, hn, count, fill, words, payload = struct.unpack("<4sIIIQQdII", raw[:48])
        assert (magic, version, dt, flags) == (b"DZMK", 1, 1 if dtype == np.float64 else 0, M.MISS_VALUE)
        assert (hn, count, fill, words, payload) == (N, int(miss.sum()), FILL, -(-N // 64), len(raw) - 48)
        w = np.frombuffer(zlib.decompress(raw[48:]), dtype=np.uint64)
        assert np.array_equal(w, M.mask_words(miss))
        d = zlib.decompressobj()
        assert len(d.decompress(raw[48:])) == 8 * words and d.eof and d.unused_data == b""        # one stream, nothing behind it
        assert payload < 8 * words
        # decode: the fill where the mask says so, the plain decode elsewhere
        out = np.empty_like(x)
        assert lib.dctz_decompress_masked(C.byref(_zvar(z, dtype)), blob, nbytes.value, None, 0, C.byref(D._tvar(out))) == 1
        assert np.array_equal(_bits(out), _bits(np.where(miss, dtype(FILL), full)))
        # ... and dctz_decompress reads the container as before
        again = np.empty_like(x)
        assert lib.dctz_decompress(C.byref(_zvar(z, dtype)), C.byref(D._tvar(again))) == 1
        assert np.array_equal(_bits(again), _bits(full))
        # with a correction list built against the FILLED array: the composed guarantee
        sf = 10.0
        bound = 0.5 * EB * sf
        fbytes = C.c_size_t(0)
        ref = filled.copy()
        assert lib.dctz_fixup_build(C.byref(_zvar(z, dtype)), C.byref(D._tvar(ref)), N, bound, C.byref(fix), C.byref(fbytes)) == 1
        listed = int(np.frombuffer(C.string_at(fix, 48)[32:40], dtype=np.uint64)[0])
        with np.errstate(invalid="ignore"):
            far = ~(np.abs(filled - full) <= dtype(bound))
        assert listed == int(far.sum()) > 0
        out2 = np.empty_like(x)
        assert lib.dctz_decompress_masked(C.byref(_zvar(z, dtype)), blob, nbytes.value, fix, fbytes.value, C.byref(D._tvar(out2))) == 1
        assert np.array_equal(_bits(out2), _bits(np.where(miss, dtype(FILL), np.where(far, filled, full))))
        same = _bits(out2) == _bits(x)
        with np.errstate(invalid="ignore", over="ignore"):
            near = np.abs(x - out2) <= dtype(bound)
        assert bool((same | near)[~miss].all()) and bool((_bits(out2)[miss] == _bits(np.array([FILL], dtype))[0]).all())
        # refusals: a blob cut short, of another array, with a damaged payload, a correction blob that does not fit
        sent = np.full_like(x, 7.0)
        for what, b in (("cut", raw[:-3]), ("n", raw[:16] + struct.pack("<Q", N + 64) + raw[24:]),
                        ("dtype", raw[:8] + struct.pack("<I", 1 - dt) + raw[12:]),
                        ("payload", raw[:48] + bytes(len(raw) - 48)),
                        ("payload of another length", raw[:44] + struct.pack("<I", len(zlib.compress(bytes(8 * words - 8), 6))) +
                         zlib.compress(bytes(8 * words - 8), 6))):
            bb = C.create_string_buffer(b, len(b))
            assert lib.dctz_decompress_masked(C.byref(_zvar(z, dtype)), bb, len(b), None, 0, C.byref(D._tvar(sent))) == -1, what
        assert lib.dctz_decompress_masked(C.byref(_zvar(z, dtype)), blob, nbytes.value, fix, fbytes.value - 8, C.byref(D._tvar(sent))) == -1
        assert (sent == 7.0).all()
    finally:
        libc.free(blob)
        libc.free(fix)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_refusals(mode):
    lib = _lib(mode)
    x, miss = _holey(np.float64)
    z = np.zeros(N * 8 + (1 << 16), np.uint8)
    sz, blob, nbytes = C.c_size_t(0), C.c_void_p(), C.c_size_t(0)

    def call(rule, buf):
        return lib.dctz_compress_masked(C.byref(D._tvar(buf)), N, C.byref(sz), C.byref(_zvar(z, np.float64)), EB,
                                        C.byref(rule) if rule is not None else None, FILL, C.byref(blob), C.byref(nbytes))

    buf = x.copy()
    for rule in (None, DMissing(0, 0, 0), DMissing(32, 0, 0), DMissing(M.MISS_VALUE, float("nan"), 0), DMissing(M.MISS_ABS_GE, 0, 0.0),
                 DMissing(M.MISS_ABS_GE, 0, float("inf"))):
        assert call(rule, buf) == -1
    # pending block dimensions: the fill runs over flat blocks only; the request stays pending and is withdrawn here
    dims = (C.c_size_t * 2)(N // 5, 5)
    assert N % 5 == 0 and lib.dctz_set_block_dims(2, dims) == 0
    assert call(DMissing(M.MISS_VALUE, 1e36, 0), buf) == -1
    assert lib.dctz_set_block_dims(0, None) == 0
    assert blob.value is None and np.array_equal(_bits(buf), _bits(x))
    # a DZND container is refused by the decode
    tiled = W.ragged(64 * 64, np.float64)
    dims = (C.c_size_t * 2)(64, 64)
    assert lib.dctz_set_block_dims(2, dims) == 0
    zt = np.zeros(tiled.size * 8 + (1 << 16), np.uint8)
    assert lib.dctz_compress(C.byref(D._tvar(tiled.copy())), tiled.size, C.byref(sz), C.byref(_zvar(zt, np.float64)), EB) == 1
    words = tiled.size // 64
    pay = zlib.compress(bytes(8 * words), 6)
    b = b"DZMK" + struct.pack("<IIIQQdII", 1, 1, M.MISS_NAN, tiled.size, 0, 0.0, words, len(pay)) + pay
    out = np.full(tiled.size, 7.0)
    assert lib.dctz_decompress_masked(C.byref(_zvar(zt, np.float64)), C.create_string_buffer(b, len(b)), len(b), None, 0, C.byref(D._tvar(out))) == -1
    assert (out == 7.0).all()
