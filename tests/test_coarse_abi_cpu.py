"""CPU-side checks of the coarse decode: dctzhip_coarse_len, dctzhip_decompress_coarse and dctzhip_decompress_coarse_nd are
exported by libdctzhip.so with the documented argument types, dctz_decompress_coarse by both drop-in libraries, the length
function has the documented values, and the device ABI refuses a NULL context before it touches a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
E_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not all(os.path.exists(os.path.join(LIB, f)) for f in ("libdctzhip.so", "libdctz-ec.so", "libdctz-qt.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, so)], text=True)
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_shim_exports_the_calls():
    ex = _exported("libdctzhip.so")
    assert {"dctzhip_coarse_len", "dctzhip_decompress_coarse", "dctzhip_decompress_coarse_nd"} <= ex
    import dctz_amd
    from dctz_amd import hip as H
    assert H.E_ARG == E_ARG
    lib = dctz_amd.load_library()
    for name in ("dctzhip_coarse_len", "dctzhip_decompress_coarse", "dctzhip_decompress_coarse_nd"):
        assert hasattr(lib, name)
    assert hasattr(H.Context, "decompress_coarse") and hasattr(H.Context, "decompress_coarse_nd")


def test_argument_types():
    """The prototypes of include/dctz_hip.h as the Python binding declares them: fourteen / fifteen arguments, the factor an
    int in front of d_out."""
    import dctz_amd
    lib = dctz_amd.load_library()
    vp = C.c_void_p
    assert lib.dctzhip_coarse_len.restype is C.c_size_t and lib.dctzhip_coarse_len.argtypes == [C.c_size_t, C.c_int]
    assert lib.dctzhip_decompress_coarse.restype is C.c_int
    assert lib.dctzhip_decompress_coarse.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_double,
                                                      C.c_int, C.c_int, vp]
    assert lib.dctzhip_decompress_coarse_nd.restype is C.c_int
    assert lib.dctzhip_decompress_coarse_nd.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_int, C.POINTER(C.c_size_t), C.c_int,
                                                         C.c_double, C.c_double, C.c_int, C.c_int, vp]
    with open(os.path.join(ROOT, "include", "dctz_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert "size_t dctzhip_coarse_len(size_t n, int factor);" in hdr
    assert "double error_bound, double sf, int mode, int factor, void *d_out);" in hdr


def test_coarse_len_values():
    import dctz_amd
    lib = dctz_amd.load_library()
    for n in (1, 37, 63, 64, 65, 4096, 4097, 3 * 4096 + 5 * 64 + 37, 2 ** 31 - 1):
        for f in (2, 4, 8, 16, 32, 64):
            assert lib.dctzhip_coarse_len(n, f) == (n + f - 1) // f, (n, f)
            # K = 64 / f values per whole block, ceil(l / f) for the short one
            assert lib.dctzhip_coarse_len(n, f) == (n // 64) * (64 // f) + (n % 64 + f - 1) // f
        for f in (0, 1, 3, 6, 48, 128, -2, -64):
            assert lib.dctzhip_coarse_len(n, f) == 0, (n, f)


def test_version_is_bumped():
    import dctz_amd
    v = dctz_amd.load_library().dctzhip_version().decode()
    assert tuple(int(p) for p in v.split(".")) >= (0, 4, 0), v


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert "dctz_decompress_coarse" in _exported(so)


def test_null_context_is_refused():
    import dctz_amd
    lib = dctz_amd.load_library()
    assert lib.dctzhip_decompress_coarse(None, None, None, None, 0, None, None, 4096, 1, 1e-3, 1.0, 0, 8, None) == E_ARG
    dims = (C.c_size_t * 3)(8, 8, 8)
    assert lib.dctzhip_decompress_coarse_nd(None, None, None, None, 0, None, None, 3, dims, 1, 1e-3, 1.0, 0, 2, None) == E_ARG
