"""CPU-side checks of the correction list for arrays compressed in 8 x 8 / 4 x 4 x 4 tiles: dctzhip_fixup_build_nd and
dctzhip_fixup_apply_nd are exported by libdctzhip.so with the documented argument types and prototypes and refuse a NULL
context before they touch a GPU; the drop-in libraries refuse a version-2 blob that does not fit its DZND container -- and a
blob of the other kind -- from the headers alone; the blob layout is written down once."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
CALLS = ("dctzhip_fixup_build_nd", "dctzhip_fixup_apply_nd")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not all(os.path.exists(os.path.join(LIB, f)) for f in ("libdctzhip.so", "libdctz-ec.so", "libdctz-qt.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return " ".join(f.read().split())


def test_shim_exports_the_calls():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, "libdctzhip.so")], text=True)
    assert set(CALLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    for name in CALLS:
        assert hasattr(lib, name)
    assert hasattr(H.Context, "fixup_build_nd") and hasattr(H.Context, "fixup_apply_nd")


def test_argument_types_and_prototypes():
    import dctz_amd
    lib = dctz_amd.load_library()
    vp, ps = C.c_void_p, C.POINTER(C.c_size_t)
    assert lib.dctzhip_fixup_build_nd.restype is C.c_int
    assert lib.dctzhip_fixup_build_nd.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_int, ps, C.c_int, C.c_double, C.c_double, C.c_int, vp,
                                                   C.c_double, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    assert lib.dctzhip_fixup_apply_nd.restype is C.c_int
    assert lib.dctzhip_fixup_apply_nd.argtypes == [vp, vp, vp, vp, C.c_uint32, C.c_int, ps, C.c_int, ps, ps, vp]
    hdr = _header("dctz_hip.h")
    assert ("int dctzhip_fixup_build_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact, "
            "uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims, const size_t *dims, int dtype, "
            "double error_bound, double sf, int mode, const void *d_ref, double bound, uint32_t *d_fix_start, "
            "uint16_t *d_fix_off /* or NULL */, void *d_fix_val /* or NULL */, uint32_t capacity, uint32_t *count /* host */);") in hdr
    assert ("int dctzhip_fixup_apply_nd(dctzhip_ctx *ctx, const uint32_t *d_fix_start, const uint16_t *d_fix_off, const void *d_fix_val, "
            "uint32_t count, int ndims, const size_t *dims, int dtype, const size_t *lo, const size_t *hi, void *d_out);") in hdr
    # no new drop-in entry points: the container decides
    hdr = _header("dctz.h")
    assert "int dctz_fixup_build(t_var *var_z, t_var *var_ref, int N_ref, double bound, void **blob, size_t *blob_bytes);" in hdr
    assert "int dctz_decompress_bounded(t_var *var_z, const void *blob, size_t blob_bytes, t_var *var_r);" in hdr
    assert "fixup_build_nd" not in hdr and "bounded_nd" not in hdr


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    count = C.c_uint32(0)
    dims = (C.c_size_t * 2)(45, 77)
    zero = (C.c_size_t * 2)(0, 0)
    assert lib.dctzhip_fixup_build_nd(None, None, None, None, 0, None, None, 2, dims, 1, 1e-3, 1.0, 0, None, 0.1, None, None, None, 0,
                                      C.byref(count)) == H.E_ARG
    assert lib.dctzhip_fixup_apply_nd(None, None, None, None, 0, 2, dims, 1, zero, dims, None) == H.E_ARG


class TVarBuf(C.Union):
    _fields_ = [("f", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_double))]


class TVar(C.Structure):   # dctz.h:49-59
    _fields_ = [("datatype", C.c_int), ("err_bound", C.c_double), ("var_name", C.c_char_p), ("buf", TVarBuf)]


def _nblk(dims):
    e = 8 if len(dims) == 2 else 4
    return int(np.prod([-(-d // e) for d in dims]))


def _blob(dims, is_d, count=0, version=2, nd=None, n=None, tiles=None, dtype=None, bound=0.1, hdims=None, cut=0):
    """A version-2 blob with the header the arguments say and a payload of zeros of the length that header describes."""
    n_true = int(np.prod(dims))
    t = -(-64 * _nblk(dims) // 4096) if tiles is None else tiles
    pad8 = lambda v: (v + 7) & ~7
    payload = pad8(4 * (t + 1)) + pad8(2 * count) + count * (8 if is_d else 4)
    head = b"DZFX" + struct.pack("<IIIQQQd", version, int(is_d) if dtype is None else dtype, len(dims) if nd is None else nd,
                                 n_true if n is None else n, t, count, bound)
    hd = list(dims if hdims is None else hdims) + [0] * 3
    head += struct.pack("<QQQ", *hd[:3])
    assert len(head) == 72
    return head + bytes(payload - cut)


def _flat_blob(n, is_d, count=0):
    tiles = -(-n // 4096)
    pad8 = lambda v: (v + 7) & ~7
    head = b"DZFX" + struct.pack("<IIIQQQd", 1, int(is_d), 0, n, tiles, count, 0.1)
    return head + bytes(pad8(4 * (tiles + 1)) + pad8(2 * count) + count * (8 if is_d else 4))


def _container(dims, is_d, qt):
    """The header of a DZND container with empty sections and its extents behind them (dctz.h: struct header; the trailer
    "DZND", dims): nothing else that could be read."""
    z = np.zeros(56 + (64 * (8 if is_d else 4) if qt else 0) + 16 + 64, np.uint8)
    put = lambda at, fmt, *v: z.__setitem__(slice(at, at + struct.calcsize(fmt)), np.frombuffer(struct.pack(fmt, *v), np.uint8))
    put(0, "<I", (1 if is_d else 0) | (len(dims) << 8))        # datatype with the geometry bits
    put(4, "<I", int(np.prod(dims)))                           # num_elements
    at = 56 + (64 * (8 if is_d else 4) if qt else 0)
    put(at, "<4sIII", b"DZND", *(list(dims) + [0])[:3])
    return z


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_a_blob_that_does_not_fit_the_container_is_refused_first(so):
    """-1 from the headers alone: no section is inflated and no device is asked for (there is none here; a call that went on
    would end the process)."""
    os.environ["DCTZ_QUIET"] = "1"
    lib = C.CDLL(os.path.join(LIB, so))
    lib.dctz_decompress_bounded.restype = C.c_int
    lib.dctz_decompress_bounded.argtypes = [C.POINTER(TVar), C.c_void_p, C.c_size_t, C.POINTER(TVar)]
    qt = "qt" in so
    dims = (100, 200)
    n = 100 * 200
    z = _container(dims, True, qt)
    zv = TVar()
    zv.datatype = 1
    zv.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(n, np.float64)
    ov = TVar()
    ov.datatype = 1
    ov.buf.d = out.ctypes.data_as(C.POINTER(C.c_double))
    good = _blob(dims, True, count=5)
    bad = {"version 1 blob": _flat_blob(n, True, 5), "version": _blob(dims, True, 5, version=3), "dtype": _blob(dims, True, 5, dtype=0),
           "ndims": _blob(dims, True, 5, nd=3), "ndims 0": _blob(dims, True, 5, nd=0), "other dims": _blob((200, 100), True, 5),
           "3-D dims": _blob((100, 200, 1), True, 5, nd=2), "n": _blob(dims, True, 5, n=n + 1), "tiles": _blob(dims, True, 5, tiles=3),
           "count": _blob(dims, True, n + 1), "bound": _blob(dims, True, 5, bound=-1.0), "nan bound": _blob(dims, True, 5, bound=float("nan")),
           "inf bound": _blob(dims, True, 5, bound=float("inf")), "short": good[:-8], "long": good + bytes(8), "header cut": good[:64],
           "flat header only": good[:48]}
    for what, b in bad.items():
        buf = C.create_string_buffer(b, len(b))
        assert lib.dctz_decompress_bounded(C.byref(zv), buf, len(b), C.byref(ov)) == -1, what
    assert lib.dctz_decompress_bounded(C.byref(zv), None, 0, C.byref(ov)) == -1
    # a version-2 blob with a flat container of the same n
    z[0:4] = np.frombuffer(struct.pack("<I", 1), np.uint8)
    buf = C.create_string_buffer(good, len(good))
    assert lib.dctz_decompress_bounded(C.byref(zv), buf, len(good), C.byref(ov)) == -1
    assert not out.any()


def test_the_good_blob_of_the_refusal_test_passes_the_check(tmp_path):
    """dzfx_check_nd itself, compiled for the host: the blob the refusals are variations of is accepted, so each refusal is
    the variation's; a flat blob passes dzfx_check as before."""
    src = tmp_path / "chk.c"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "dctz_fixup_blob.h"\n'
                   'int main(int argc, char **argv) {\n'
                   '  FILE *f = fopen(argv[1], "rb"); static unsigned char b[1 << 16]; size_t k = fread(b, 1, sizeof(b), f); fclose(f);\n'
                   '  size_t dims[3] = {100, 200, 0}; dzfx_header_nd h; dzfx_header h1;\n'
                   '  printf("%d %d %u %zu\\n", dzfx_check_nd(b, k, 1, 2, dims, 20000, 13 * 25, &h), dzfx_check(b, k, 1, 20000, &h1),\n'
                   '         dzfx_version(b, k), dzfx_header_bytes(dzfx_version(b, k)));\n'
                   '  return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "dctz_amd", "csrc"), "-o", str(exe), str(src), "-lm"])
    p = tmp_path / "blob"
    p.write_bytes(_blob((100, 200), True, count=5))
    assert subprocess.check_output([str(exe), str(p)], text=True).split() == ["0", "-1", "2", "72"]
    p.write_bytes(_flat_blob(20000, True, 5))
    assert subprocess.check_output([str(exe), str(p)], text=True).split() == ["-1", "0", "1", "48"]


def test_the_blob_layout_is_written_down_once():
    """csrc/dctz_fixup_blob.h holds both layouts; the library includes it and spells no offset of its own."""
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "dctz_fixup_blob.h")) as f:
        hdr = f.read()
    assert "#define DZFX_HEADER_BYTES 48" in hdr and "#define DZFX_HEADER_BYTES_ND 72" in hdr and "#define DZFX_VERSION_ND 2u" in hdr
    assert "dzfx_check_nd(" in hdr and "dzfx_check(" in hdr
    with open(os.path.join(ROOT, "dctz_amd", "csrc", "libdctz.c")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert '#include "dctz_fixup_blob.h"' in src and '"DZFX"' not in src
    assert "dzfx_check_nd(" in src and "dzfx_write_header_nd(" in src
    # the library names the header's size only through the blob header's own function and constants
    assert not re.search(r"\b(48|72)\b", "\n".join(l for l in src.splitlines() if "dzfx" in l or "DZFX" in l))
