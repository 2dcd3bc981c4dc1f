"""CPU-side checks of the point-wise error bound: dctzhip_fixup_tiles, dctzhip_fixup_build and dctzhip_fixup_apply are exported
by libdctzhip.so with the documented argument types, dctz_fixup_build and dctz_decompress_bounded by both drop-in libraries;
DCTZHIP_E_SPACE is appended to the error codes and the others keep their values; the device ABI refuses a NULL context and
NULL pointers before it touches a GPU; the drop-in refuses a blob whose header does not fit the container before anything else."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
CALLS = ("dctzhip_fixup_tiles", "dctzhip_fixup_build", "dctzhip_fixup_apply")


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
    assert hasattr(H.Context, "fixup_build") and hasattr(H.Context, "fixup_apply")


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_calls(so):
    assert {"dctz_fixup_build", "dctz_decompress_bounded"} <= _exported(so)


def test_argument_types_and_prototypes():
    import dctz_amd
    lib = dctz_amd.load_library()
    vp = C.c_void_p
    assert lib.dctzhip_fixup_tiles.restype is C.c_size_t and lib.dctzhip_fixup_tiles.argtypes == [C.c_size_t]
    assert lib.dctzhip_fixup_build.restype is C.c_int
    assert lib.dctzhip_fixup_build.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, vp,
                                                C.c_double, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    assert lib.dctzhip_fixup_apply.restype is C.c_int
    ps = C.POINTER(C.c_size_t)
    assert lib.dctzhip_fixup_apply.argtypes == [vp, vp, vp, vp, C.c_uint32, C.c_size_t, C.c_int, C.c_int, ps, ps, ps, vp]
    hdr = _header("dctz_hip.h")
    assert "size_t dctzhip_fixup_tiles(size_t n);" in hdr
    assert ("int dctzhip_fixup_build(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact, "
            "uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype, double error_bound, double sf, "
            "int mode, const void *d_ref, double bound, uint32_t *d_fix_start, uint16_t *d_fix_off /* or NULL */, "
            "void *d_fix_val /* or NULL */, uint32_t capacity, uint32_t *count /* host */);") in hdr
    assert ("int dctzhip_fixup_apply(dctzhip_ctx *ctx, const uint32_t *d_fix_start, const uint16_t *d_fix_off, const void *d_fix_val, "
            "uint32_t count, size_t n, int dtype, int ndim, const size_t *dims, const size_t *lo, const size_t *hi, void *d_out);") in hdr
    hdr = _header("dctz.h")
    assert "int dctz_fixup_build(t_var *var_z, t_var *var_ref, int N_ref, double bound, void **blob, size_t *blob_bytes);" in hdr
    assert "int dctz_decompress_bounded(t_var *var_z, const void *blob, size_t blob_bytes, t_var *var_r);" in hdr


def test_error_codes(tmp_path):
    """DCTZHIP_E_SPACE is appended; the existing values are unchanged -- by the C compiler and in the binding."""
    from dctz_amd import hip as H
    assert (H.OK, H.E_ARG, H.E_BOUND, H.E_HIP, H.E_INTERNAL, H.E_SPACE) == (0, -1, -2, -3, -4, -5)
    src = tmp_path / "codes.c"
    src.write_text('#include <stdio.h>\n#include "dctz_hip.h"\nint main(void) { printf("%d %d %d %d %d %d\\n", DCTZHIP_OK, DCTZHIP_E_ARG, '
                   'DCTZHIP_E_BOUND, DCTZHIP_E_HIP, DCTZHIP_E_INTERNAL, DCTZHIP_E_SPACE); return 0; }\n')
    exe = tmp_path / "codes"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["0", "-1", "-2", "-3", "-4", "-5"]
    hdr = _header("dctz_hip.h")
    order = [hdr.index(k) for k in ("DCTZHIP_OK = 0", "DCTZHIP_E_ARG = -1", "DCTZHIP_E_BOUND = -2", "DCTZHIP_E_HIP = -3", "DCTZHIP_E_INTERNAL = -4",
                                    "DCTZHIP_E_SPACE = -5")]
    assert order == sorted(order)


def test_fixup_tiles_values():
    import dctz_amd
    lib = dctz_amd.load_library()
    for n, want in ((1, 1), (4096, 1), (4097, 2), (2 ** 31 - 1, 2 ** 19)):
        assert lib.dctzhip_fixup_tiles(n) == want, n
    for n in (37, 63, 64, 8192, 3 * 4096 + 5 * 64 + 37):
        assert lib.dctzhip_fixup_tiles(n) == lib.dctzhip_summary_tiles(n) == -(-n // 4096), n


def test_null_context_and_null_pointers_are_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    count = C.c_uint32(0)
    one = (C.c_size_t * 1)(4096)
    zero = (C.c_size_t * 1)(0)
    assert lib.dctzhip_fixup_build(None, None, None, None, 0, None, None, 4096, 1, 1e-3, 1.0, 0, None, 0.1, None, None, None, 0,
                                   C.byref(count)) == H.E_ARG
    assert lib.dctzhip_fixup_apply(None, None, None, None, 0, 4096, 1, 1, one, zero, one, None) == H.E_ARG


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


def _blob(n, is_d, count=0, magic=b"DZFX", version=1, dtype=None, bound=0.1, cut=0):
    tiles = -(-n // 4096)
    pad8 = lambda v: (v + 7) & ~7
    payload = pad8(4 * (tiles + 1)) + pad8(2 * count) + count * (8 if is_d else 4)
    head = magic + struct.pack("<IIIQQQd", version, int(is_d) if dtype is None else dtype, 0, n, tiles, count, bound)
    assert len(head) == 48
    return head + bytes(payload - cut)


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_a_blob_that_does_not_fit_the_container_is_refused_first(so):
    """-1 from the two headers alone: no section is inflated and no device is asked for (there is none here; a call that went
    on would end the process)."""
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    lib.dctz_decompress_bounded.restype = C.c_int
    lib.dctz_decompress_bounded.argtypes = [C.POINTER(TVar), C.c_void_p, C.c_size_t, C.POINTER(TVar)]
    n = 3 * 4096 + 37
    # 56 header bytes of a flat fp64 container of n elements (dctz.h: struct header), nothing behind them that could be read
    z = np.zeros(64, np.uint8)
    z[0:4] = np.frombuffer(struct.pack("<I", 1), np.uint8)            # datatype DOUBLE, flat blocks
    z[4:8] = np.frombuffer(struct.pack("<I", n), np.uint8)            # num_elements
    zv = TVar()
    zv.datatype = 1
    zv.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(n, np.float64)
    ov = TVar()
    ov.datatype = 1
    ov.buf.d = out.ctypes.data_as(C.POINTER(C.c_double))
    good = _blob(n, True, count=5)
    bad = {"magic": _blob(n, True, 5, magic=b"DZFY"), "version": _blob(n, True, 5, version=2), "dtype": _blob(n, True, 5, dtype=0),
           "n": _blob(n + 1, True, 5), "short": good[:-8], "long": good + bytes(8), "header cut": good[:40], "count": _blob(n, True, n + 1),
           "bound": _blob(n, True, 5, bound=-1.0), "nan bound": _blob(n, True, 5, bound=float("nan"))}
    for what, b in bad.items():
        buf = C.create_string_buffer(b, len(b))
        assert lib.dctz_decompress_bounded(C.byref(zv), buf, len(b), C.byref(ov)) == -1, what
    assert lib.dctz_decompress_bounded(C.byref(zv), None, 0, C.byref(ov)) == -1
    # the tile count is part of the fit
    tiles_off = bytearray(good)
    tiles_off[24:32] = struct.pack("<Q", 3)
    buf = C.create_string_buffer(bytes(tiles_off), len(tiles_off))
    assert lib.dctz_decompress_bounded(C.byref(zv), buf, len(tiles_off), C.byref(ov)) == -1
    # a DZND container is out of scope whatever the blob says
    z[0:4] = np.frombuffer(struct.pack("<I", 1 | (2 << 8)), np.uint8)
    buf = C.create_string_buffer(good, len(good))
    assert lib.dctz_decompress_bounded(C.byref(zv), buf, len(good), C.byref(ov)) == -1
    assert not out.any()


def test_the_blob_layout_is_written_down_once():
    """csrc/dctz_fixup_blob.h holds the layout; the library includes it and spells no offset of its own."""
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "dctz_fixup_blob.h")) as f:
        hdr = f.read()
    assert '#define DZFX_MAGIC "DZFX"' in hdr and "#define DZFX_HEADER_BYTES 48" in hdr
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "libdctz.c")) as f:
        src = f.read()
    assert '#include "dctz_fixup_blob.h"' in src and '"DZFX"' not in re.sub(r"/\*.*?\*/", "", src, flags=re.S)
