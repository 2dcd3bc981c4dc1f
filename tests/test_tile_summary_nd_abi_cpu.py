"""CPU-side checks of the tile summaries for tiled arrays: dctzhip_tile_summary_nd is exported by libdctzhip.so with the
documented argument types, dctz_tile_summary_nd by both drop-in libraries, the declarations stand in the headers, the Python
binding has the method, and the device ABI refuses a NULL context before it touches a GPU."""
import ctypes as C
import inspect
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
    assert "dctzhip_tile_summary_nd" in _exported("libdctzhip.so")
    import dctz_amd
    from dctz_amd import hip as H
    assert hasattr(dctz_amd.load_library(), "dctzhip_tile_summary_nd")
    assert hasattr(H.Context, "tile_summary_nd")
    assert list(inspect.signature(H.Context.tile_summary_nd).parameters) == [
        "self", "out", "cnt", "shape", "dtype", "eb", "sf", "index", "mode", "qtable", "ref"]


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert {"dctz_tile_summary_nd", "dctz_tile_summary"} <= _exported(so)


def test_argument_types_and_prototypes():
    """The prototype of include/dctz_hip.h as the Python binding declares it: sixteen arguments, ndims and dims where the flat
    call has n; the record type is the flat call's."""
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    vp = C.c_void_p
    assert lib.dctzhip_tile_summary_nd.restype is C.c_int
    assert lib.dctzhip_tile_summary_nd.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double,
                                                    C.c_double, C.c_int, vp, vp, C.POINTER(H.TileSummary)]
    with open(os.path.join(ROOT, "include", "dctz_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert ("int dctzhip_tile_summary_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact, "
            "uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims, const size_t *dims, int dtype, "
            "double error_bound, double sf, int mode, const void *d_ref /* or NULL */, dctzhip_tile_summary_t *d_tiles /* or NULL */, "
            "dctzhip_tile_summary_t *total /* host, or NULL */);") in hdr
    assert "dctzhip_tile_summary_nd below" in hdr         # the flat call's comment points at it
    with open(os.path.join(ROOT, "include", "dctz.h")) as f:
        hdr = " ".join(f.read().split())
    assert ("int dctz_tile_summary_nd(t_var *var_z, t_var *var_ref /* or NULL */, int N_ref, dctz_tile_summary_t *tiles /* host, or NULL */, "
            "dctz_tile_summary_t *total);") in hdr


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    total = H.TileSummary()
    dims = (C.c_size_t * 2)(64, 64)
    assert lib.dctzhip_tile_summary_nd(None, None, None, None, 0, None, None, 2, dims, 1, 1e-3, 1.0, 0, None, None, C.byref(total)) == E_ARG
