"""CPU-side checks of the list form of the coarse box decode: dctzhip_decompress_coarse_boxes_nd is exported by libdctzhip.so
with the header's argument types, dctz_decompress_coarse_boxes_nd by both drop-in libraries, the Python method exists, and
the device ABI refuses a NULL context before it touches a GPU."""
import ctypes as C
import os
import re
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
    assert "dctzhip_decompress_coarse_boxes_nd" in _exported("libdctzhip.so")
    import dctz_amd
    from dctz_amd import hip as H
    assert H.E_ARG == E_ARG
    assert hasattr(dctz_amd.load_library(), "dctzhip_decompress_coarse_boxes_nd")
    assert hasattr(H.Context, "decompress_coarse_boxes_nd")


CTYPE = {"dctzhip_ctx *": C.c_void_p, "const void *": C.c_void_p, "void *": C.c_void_p, "const float *": C.c_void_p,
         "const uint32_t *": C.c_void_p, "uint32_t": C.c_uint32, "int": C.c_int, "double": C.c_double,
         "const size_t *": C.POINTER(C.c_size_t), "const dctzhip_box_item *": C.c_void_p}


def test_argument_types_are_the_headers():
    """The prototype of include/dctz_hip.h, parameter by parameter, against the ctypes declaration: dctzhip_decompress_coarse_nd's
    up to the factor, then dctzhip_decompress_boxes_nd's k and boxes."""
    import dctz_amd
    lib = dctz_amd.load_library()
    with open(os.path.join(ROOT, "include", "dctz_hip.h")) as f:
        hdr = " ".join(f.read().split())
    m = re.search(r"int dctzhip_decompress_coarse_boxes_nd\(([^)]*)\);", hdr)
    assert m
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).split(",")]
    types = [re.sub(r"\w+$", "", p).strip() for p in params]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "d_bin_index", "d_dc", "d_ac_exact", "ac_count", "d_index", "qtable_host", "ndims", "dims", "dtype",
                     "error_bound", "sf", "mode", "factor", "k", "boxes"]
    fn = lib.dctzhip_decompress_coarse_boxes_nd
    assert fn.restype is C.c_int
    assert fn.argtypes == [CTYPE[t] for t in types]
    assert fn.argtypes[:14] == lib.dctzhip_decompress_coarse_nd.argtypes[:14]
    assert fn.argtypes[14:] == lib.dctzhip_decompress_boxes_nd.argtypes[-2:]
    assert ("int dctz_decompress_coarse_boxes_nd(t_var *var_z, int factor, int k, const size_t *lo, const size_t *hi, "
            "t_var *const *var_r);") in " ".join(open(os.path.join(ROOT, "include", "dctz.h")).read().split())


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert "dctz_decompress_coarse_boxes_nd" in _exported(so)


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    dims = (C.c_size_t * 3)(8, 8, 8)
    items = (H.BoxItem * 1)()
    for i in range(3):
        items[0].lo[i], items[0].hi[i] = 0, 1
    assert lib.dctzhip_decompress_coarse_boxes_nd(None, None, None, None, 0, None, None, 3, dims, 1, 1e-3, 1.0, 0, 2, 1,
                                                  C.cast(items, C.c_void_p)) == E_ARG
