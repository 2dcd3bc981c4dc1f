"""Command-line harness (dctz_amd/cli): the reference's argv / stdout / file-name contract
(dctz-test.c:40-103, 183-184, 222-283; tools/dctz-dump.c:41-50) on top of the drop-in library."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from tests.containers import container as _container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dctz_amd", "bin")


def _ensure_built():
    if not os.path.exists(os.path.join(BIN, "dctz-dump")):
        import __graft_entry__ as g
        g.build()


def test_usage_texts():
    _ensure_built()
    for exe in ("dctz-ec-test", "dctz-qt-test"):
        r = subprocess.run([os.path.join(BIN, exe)], capture_output=True, text=True)
        assert r.returncode == 0                                  # dctz-test.c:49: exit(0)
        assert r.stdout.startswith(f"Test case: {os.path.join(BIN, exe)} -d|-f [err bound] [var name] [srcFilePath] [dimension sizes...]")
    r = subprocess.run([os.path.join(BIN, "dctz-dump")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("Usage: ")


@pytest.mark.parametrize("mode", [O.EC, O.QT])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dump_reads_both_variants(tmp_path, mode, dtype):
    _ensure_built()
    x = W.ragged(64 * 40 + 17, dtype, scale=37.0)
    blob, c = _container(x, 1e-3, mode)
    f = tmp_path / "a.z"
    f.write_bytes(blob)
    r = subprocess.run([os.path.join(BIN, "dctz-dump"), str(f)], capture_output=True, text=True)
    assert r.stdout.splitlines() == [                              # tools/dctz-dump.c:41-50
        f"File Name={f}", f"data type={'double' if dtype == np.float64 else 'float'}", f"N={x.size}",
        "error_bound=0.001000", f"total # of AC_exact={c.cnt}", f"SF={c.sf:f}"]
    r = subprocess.run([os.path.join(BIN, "dctz-dump"), "-v", str(f)], capture_output=True, text=True)
    assert r.returncode == 0
    assert f"variant={'qt' if mode == O.QT else 'ec'}" in r.stdout and "= layout" in r.stdout
    if mode == O.QT:
        assert "qtable[1..4]=" + ", ".join(f"{float(v):.9g}" for v in c.qtable[1:5]) in r.stdout
    (tmp_path / "cut.z").write_bytes(blob[:-5])                    # truncated file: the bounds check must say so
    r = subprocess.run([os.path.join(BIN, "dctz-dump"), "-v", str(tmp_path / "cut.z")], capture_output=True, text=True)
    assert r.returncode == 2 and "LAYOUT MISMATCH" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["ec", "qt"])
@pytest.mark.parametrize("case", ["c1_f64", "f32_2d"])
def test_cli_harness_matches_the_reference_contract(tmp_path, variant, case):
    _ensure_built()
    mode = O.QT if variant == "qt" else O.EC
    if case == "c1_f64":
        x, flag, dims, eb_text = W.c1(), "-d", ["1048576"], "1E-3"
    else:
        x, flag, dims, eb_text = W.ragged(360 * 180, np.float32, scale=37.0), "-f", ["360", "180"], "1E-4"
    src = tmp_path / "field.bin"
    src.write_bytes(x.tobytes())
    env = dict(os.environ)
    env.pop("DCTZ_QUIET", None)
    r = subprocess.run([os.path.join(BIN, f"dctz-{variant}-test"), flag, eb_text, "var", str(src)] + dims,
                       capture_output=True, text=True, env=env, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    zpath = f"{src}.{variant}.{eb_text}.z"
    assert out[0] == f"total number of elements = {x.size}"
    assert any(l.startswith("outSize = ") for l in out)                         # library chatter, dctz-comp-lib.c:841-843
    d = dims + ["0"] * (4 - len(dims))
    assert (f"oriFilePath = {src}, outputFilePath = {zpath}, datatype = {'double' if flag == '-d' else 'float'}, "
            f"error = {eb_text}, dim1 = {d[0]}, dim2 = {d[1]}, dim3 = {d[2]}, dim4 = {d[3]}") in out
    assert any(l.startswith("uncompressed bin_index size is: ") for l in out)   # dctz-decomp-lib.c:260-262
    assert out[-1] == "done"

    eb = float(eb_text)
    c = O.compress(x, eb, mode, O.FAST)
    z = open(zpath, "rb").read()
    assert f"outsize = {len(z)}" in out
    s0, s1, s2 = struct.unpack_from("<III", z, 40)
    assert zlib.decompress(z[56:56 + s0]) == c.bin_index.tobytes()
    assert zlib.decompress(z[56 + s0 + s1:56 + s0 + s1 + s2]) == c.ac_exact.tobytes()
    rec = np.frombuffer(open(zpath + ".r", "rb").read(), dtype=x.dtype)
    ref = O.decompress(c, O.FAST)
    assert np.array_equal(rec.view(np.uint8), ref.view(np.uint8))
    p = O.psnr((x / x.dtype.type(c.sf)) * x.dtype.type(c.sf), rec)
    assert out[-2] == f"CR = {x.nbytes / len(z):.2f}, PSNR = {p['psnr']:.2f}"
    if case == "c1_f64" and variant == "ec":
        assert out[-2].endswith("PSNR = 96.38")                                  # SURVEY 8c known answer
        if zlib.ZLIB_VERSION.startswith("1.2.11"):
            assert len(z) == 3763394 and out[-2].startswith("CR = 2.23")
    d = subprocess.run([os.path.join(BIN, "dctz-dump"), "-v", zpath], capture_output=True, text=True)
    assert d.returncode == 0 and f"total # of AC_exact={c.cnt}" in d.stdout and f"variant={variant}" in d.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["ec", "qt"])
def test_cli_harness_with_the_entropy_stage_on_the_gpu(tmp_path, variant):
    """The unchanged harness under DCTZ_ZLIB_GPU=1: same stdout contract, sections that zlib inflates to the oracle's
    streams, the same `.z.r` as the default tail, a container dctz-dump accepts (chunk index shown)."""
    _ensure_built()
    mode = O.QT if variant == "qt" else O.EC
    x = W.ragged(64 * 4000 + 9, np.float64, scale=410.0)
    src = tmp_path / "field.bin"
    src.write_bytes(x.tobytes())
    env = dict(os.environ, DCTZ_ZLIB_GPU="1")
    env.pop("DCTZ_QUIET", None)
    r = subprocess.run([os.path.join(BIN, f"dctz-{variant}-test"), "-d", "1E-3", "var", str(src), str(x.size)],
                       capture_output=True, text=True, env=env, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    zpath = f"{src}.{variant}.1E-3.z"
    z = open(zpath, "rb").read()
    assert out[-1] == "done" and f"outsize = {len(z)}" in out
    c = O.compress(x, 1e-3, mode, O.FAST)
    s0, s1, s2 = struct.unpack_from("<III", z, 40)
    assert z[56:58] == b"\x78\x5e" and zlib.decompress(z[56:56 + s0]) == c.bin_index.tobytes()
    assert zlib.decompress(z[56 + s0:56 + s0 + s1]) == c.dc.tobytes()
    assert zlib.decompress(z[56 + s0 + s1:56 + s0 + s1 + s2]) == c.ac_exact.tobytes()
    rec = np.frombuffer(open(zpath + ".r", "rb").read(), dtype=x.dtype)
    assert np.array_equal(rec.view(np.uint8), O.decompress(c, O.FAST).view(np.uint8))
    d = subprocess.run([os.path.join(BIN, "dctz-dump"), "-v", zpath], capture_output=True, text=True)
    assert d.returncode == 0 and "chunk index tiles the three streams" in d.stdout and f"variant={variant}" in d.stdout and "= layout" in d.stdout, d.stdout


@pytest.mark.parametrize("mode", [O.EC, O.QT])
def test_container_check(mode):
    """dctz_check_container: the bounds / plausibility check a caller runs before dctz_decompress
    (which trusts the header like the reference, dctz-decomp-lib.c:84-100).  Host only."""
    import ctypes as C
    _ensure_built()
    lib = C.CDLL(os.path.join(ROOT, "dctz_amd", "lib", f"libdctz-{'qt' if mode == O.QT else 'ec'}.so"))
    lib.dctz_check_container.restype = C.c_int
    lib.dctz_check_container.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
    x = W.ragged(64 * 50 + 9, np.float64, scale=37.0)
    blob, c = _container(x, 1e-3, mode)
    chk = lambda b, nmax=0, deep=1: lib.dctz_check_container(bytes(b), len(b), nmax, deep)
    assert chk(blob) == 0 and chk(blob, x.size) == 0 and chk(blob + b"\0" * 7) == 0
    assert chk(blob, x.size - 1) == -3                                      # caller's buffer too small
    assert chk(blob[:40]) == -1 and chk(blob[:-1]) == -1                    # truncated
    bad = bytearray(blob); struct.pack_into("<I", bad, 0, 7); assert chk(bad) == -2          # datatype
    bad = bytearray(blob); struct.pack_into("<I", bad, 4, 0); assert chk(bad) == -2          # N = 0
    bad = bytearray(blob); struct.pack_into("<d", bad, 8, 1e-9); assert chk(bad) == -2       # error bound
    bad = bytearray(blob); struct.pack_into("<I", bad, 16, x.size); assert chk(bad) == -2    # cnt > N - nblk
    bad = bytearray(blob); struct.pack_into("<I", bad, 40, len(blob)); assert chk(bad) == -1 # section runs past the end
    bad = bytearray(blob); bad[56 + 20] ^= 0x5A; assert chk(bad, 0, 0) == 0 and chk(bad) == -4   # corrupt deflate data
    bad = bytearray(blob); struct.pack_into("<I", bad, 4, x.size + 64); assert chk(bad) in (-2, -4)  # N does not match the streams
    other = _container(x, 1e-3, O.EC if mode == O.QT else O.QT)[0]
    assert chk(other) != 0 or mode == O.EC                                   # an EC library does not see a QT file's table as an error
