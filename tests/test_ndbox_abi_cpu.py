"""CPU-side checks of the box decode of tiled arrays: dctzhip_decompress_box_nd is exported by libdctzhip.so,
dctz_decompress_box_nd by both drop-in libraries, and the device ABI refuses a NULL context before it touches a GPU."""
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


def test_shim_exports_the_call():
    assert "dctzhip_decompress_box_nd" in _exported("libdctzhip.so")
    import dctz_amd
    from dctz_amd import hip as H
    assert H.E_ARG == E_ARG
    assert hasattr(dctz_amd.load_library(), "dctzhip_decompress_box_nd") and hasattr(H.Context, "decompress_box_nd")


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert "dctz_decompress_box_nd" in _exported(so)


def test_null_context_is_refused():
    import dctz_amd
    lib = dctz_amd.load_library()
    dims = (C.c_size_t * 3)(8, 8, 8)
    lo, hi = (C.c_size_t * 3)(0, 0, 0), (C.c_size_t * 3)(1, 1, 1)
    assert lib.dctzhip_decompress_box_nd(None, None, None, None, 0, None, None, 3, dims, 1, 1e-3, 1.0, 0, lo, hi, None) == E_ARG
