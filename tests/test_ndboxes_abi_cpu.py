"""CPU-side checks of the list-of-boxes decode for tiled arrays: dctzhip_decompress_boxes_nd is exported by libdctzhip.so
and declared in include/dctz_hip.h, dctz_decompress_boxes_nd is exported by both drop-in libraries and declared in
include/dctz.h, Context.decompress_boxes_nd exists, and the device ABI refuses a NULL context before it touches a GPU."""
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


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_shim_exports_and_declares_the_call():
    assert "dctzhip_decompress_boxes_nd" in _exported("libdctzhip.so")
    assert re.search(r"\bint\s+dctzhip_decompress_boxes_nd\s*\(", _header("dctz_hip.h"))
    import dctz_amd
    from dctz_amd import hip as H
    assert H.E_ARG == E_ARG
    assert hasattr(dctz_amd.load_library(), "dctzhip_decompress_boxes_nd") and hasattr(H.Context, "decompress_boxes_nd")


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_and_declares_the_call(so):
    assert "dctz_decompress_boxes_nd" in _exported(so)
    assert re.search(r"\bint\s+dctz_decompress_boxes_nd\s*\(", _header("dctz.h"))


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    dims = (C.c_size_t * 3)(8, 8, 8)
    item = (H.BoxItem * 1)()
    for i in range(3):
        item[0].hi[i] = 1
    assert lib.dctzhip_decompress_boxes_nd(None, None, None, None, 0, None, None, 3, dims, 1, 1e-3, 1.0, 0, 1,
                                           C.cast(item, C.c_void_p)) == E_ARG
