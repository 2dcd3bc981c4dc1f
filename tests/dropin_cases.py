"""Containers and checks shared by the drop-in tests (tests/test_gpu_*_dropin.py): t_var, the two builds of the library, a
container with the zlib tail or the DZIX chunk index, flat or in tiles, one dctz_decompress_box call, the sections of a
container.  They live here so that no test file depends on another test file; each test file sets the argtypes of the
calls it tests on top of _lib."""
import ctypes as C
import os
import struct

import numpy as np

from tests import workloads as W

LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dctz_amd", "lib")
TILE = 4096
IX_MAGIC = 0x58495A44                                  # "DZIX"


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


def _lib(mode):
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIBDIR, f"libdctz-{mode}.so"))
    lib.dctz_compress.restype = C.c_int
    lib.dctz_compress.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(TVar), C.c_double]
    lib.dctz_decompress.restype = C.c_int
    lib.dctz_decompress.argtypes = [C.POINTER(TVar), C.POINTER(TVar)]
    lib.dctz_decompress_box.restype = C.c_int
    lib.dctz_decompress_box.argtypes = [C.POINTER(TVar), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                        C.POINTER(TVar)]
    lib.dctz_set_block_dims.restype = C.c_int
    lib.dctz_set_block_dims.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    return lib


def _tvar(arr):
    v = TVar()
    v.datatype = 1 if arr.dtype == np.float64 else 0
    if arr.dtype == np.float64:
        v.buf.d = arr.ctypes.data_as(C.POINTER(C.c_double))
    else:
        v.buf.f = arr.ctypes.data_as(C.POINTER(C.c_float))
    return v


def _container(lib, x, eb, gpu_tail, shape=None):
    """(container bytes as a uint8 array, the full dctz_decompress result); shape: a DZND container in tiles of that shape."""
    if gpu_tail:
        os.environ["DCTZ_ZLIB_GPU"] = "1"
    try:
        xin = x.copy()                                  # (dctz_compress scales its input in place)
        z = np.zeros(x.size * x.itemsize + (1 << 16), np.uint8)
        zv = _tvar(z.view(x.dtype)[: z.size // x.itemsize])
        sz = C.c_size_t(0)
        if shape is not None:
            assert lib.dctz_set_block_dims(len(shape), (C.c_size_t * len(shape))(*shape)) == 0
        assert lib.dctz_compress(C.byref(_tvar(xin)), x.size, C.byref(sz), C.byref(zv), eb) == 1
    finally:
        os.environ.pop("DCTZ_ZLIB_GPU", None)
    if shape is not None:
        assert (struct.unpack_from("<I", z, 0)[0] >> 8) & 0xFF == len(shape)      # a DZND container
    full = np.empty_like(x)
    assert lib.dctz_decompress(C.byref(zv), C.byref(_tvar(full))) == 1
    return z, full


def _box(lib, z, dtype, dims, lo, hi):
    ext = [max(h - l, 0) for l, h in zip(lo, hi)]
    out = np.full(max(int(np.prod(ext)), 1), np.nan, dtype)
    arr = lambda v: (C.c_size_t * len(v))(*v)
    rc = lib.dctz_decompress_box(C.byref(_tvar(z.view(dtype)[: z.size // np.dtype(dtype).itemsize])), len(dims), arr(dims), arr(lo), arr(hi),
                                 C.byref(_tvar(out)))
    return rc, out[: int(np.prod(ext))].reshape(ext) if rc == 1 else out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sl(full, dims, lo, hi):
    return full.reshape(dims)[tuple(slice(l, h) for l, h in zip(lo, hi))]


def _sections(z, dtype, qt):
    dt, n, eb, cnt = struct.unpack_from("<IIdI", z, 0)
    sizes = struct.unpack_from("<III", z, 40)
    offs = [56, 56 + sizes[0], 56 + sizes[0] + sizes[1]]
    end = offs[2] + sizes[2] + (64 * np.dtype(dtype).itemsize if qt else 0)
    if (dt >> 8) & 0xFF:
        end += 16                                        # "DZND" and its three extents
    return n, cnt, sizes, offs, end
