"""CPU-side checks of the tile summaries: dctzhip_summary_tiles and dctzhip_tile_summary are exported by libdctzhip.so with the
documented argument types, dctz_tile_summary by both drop-in libraries, a record is 64 bytes, the tile count has the
documented values, and the device ABI refuses a NULL context before it touches a GPU."""
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
    assert {"dctzhip_summary_tiles", "dctzhip_tile_summary"} <= _exported("libdctzhip.so")
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    for name in ("dctzhip_summary_tiles", "dctzhip_tile_summary"):
        assert hasattr(lib, name)
    assert hasattr(H.Context, "tile_summary") and hasattr(H.TileSummary, "psnr")


@pytest.mark.parametrize("so", ["libdctz-ec.so", "libdctz-qt.so"])
def test_dropin_exports_the_call(so):
    assert "dctz_tile_summary" in _exported(so)


def test_argument_types_and_prototypes():
    """The prototypes of include/dctz_hip.h as the Python binding declares them: fifteen arguments, the original, the records
    and the total behind the mode."""
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    vp = C.c_void_p
    assert lib.dctzhip_summary_tiles.restype is C.c_size_t and lib.dctzhip_summary_tiles.argtypes == [C.c_size_t]
    assert lib.dctzhip_tile_summary.restype is C.c_int
    assert lib.dctzhip_tile_summary.argtypes == [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int,
                                                 vp, vp, C.POINTER(H.TileSummary)]
    with open(os.path.join(ROOT, "include", "dctz_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert "size_t dctzhip_summary_tiles(size_t n);" in hdr
    assert ("int dctzhip_tile_summary(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact, "
            "uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype, double error_bound, "
            "double sf, int mode, const void *d_ref /* or NULL */, dctzhip_tile_summary_t *d_tiles /* or NULL */, "
            "dctzhip_tile_summary_t *total /* host, or NULL */);") in hdr
    assert "double rmin, rmax;" in hdr and "double rsum, rsq;" in hdr and "double xmin, xmax;" in hdr and "double emax, esq;" in hdr
    with open(os.path.join(ROOT, "include", "dctz.h")) as f:
        hdr = " ".join(f.read().split())
    assert ("int dctz_tile_summary(t_var *var_z, t_var *var_ref /* or NULL */, int N_ref, dctz_tile_summary_t *tiles /* host, or NULL */, "
            "dctz_tile_summary_t *total);") in hdr


def test_a_record_is_64_bytes(tmp_path):
    """sizeof of the C type, by the C compiler, for both headers; the binding's structure has the same size and field order."""
    from dctz_amd import hip as H
    assert C.sizeof(H.TileSummary) == 64
    assert [f for f, _ in H.TileSummary._fields_] == ["rmin", "rmax", "rsum", "rsq", "xmin", "xmax", "emax", "esq"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "dctz_hip.h"\n#include "dctz.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(dctzhip_tile_summary_t), sizeof(dctz_tile_summary_t)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["64", "64"]


def test_summary_tiles_values():
    import dctz_amd
    lib = dctz_amd.load_library()
    for n, want in ((1, 1), (4096, 1), (4097, 2), (2 ** 31 - 1, 2 ** 19)):
        assert lib.dctzhip_summary_tiles(n) == want, n
    for n in (37, 63, 64, 8192, 3 * 4096 + 5 * 64 + 37):
        assert lib.dctzhip_summary_tiles(n) == -(-n // 4096), n


def test_null_context_is_refused():
    import dctz_amd
    from dctz_amd import hip as H
    lib = dctz_amd.load_library()
    total = H.TileSummary()
    assert lib.dctzhip_tile_summary(None, None, None, None, 0, None, None, 4096, 1, 1e-3, 1.0, 0, None, None, C.byref(total)) == E_ARG
