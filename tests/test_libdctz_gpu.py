"""The drop-in boundary: dctz_compress() / dctz_decompress() of lib/libdctz-{ec,qt}.so
called exactly the way dctz-test.c calls them (dctz-test.c:130-181, 250), checked
against the oracle and the survey's known answers."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import nonfinite as NF
from tests import workloads as W

pytestmark = pytest.mark.gpu
LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dctz_amd", "lib")


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
    lib.calc_psnr.restype = C.c_double
    return lib


def _tvar(arr):
    v = TVar()
    v.datatype = 1 if arr.dtype == np.float64 else 0
    if arr.dtype == np.float64:
        v.buf.d = arr.ctypes.data_as(C.POINTER(C.c_double))
    else:
        v.buf.f = arr.ctypes.data_as(C.POINTER(C.c_float))
    return v


def _parse(z, dtype, qt):
    # struct header, dctz.h:96-119 (56 bytes, native endianness; offsets SURVEY 8b)
    dt, n, eb, cnt = struct.unpack_from("<IIdI", z, 0)
    sf = struct.unpack_from("<d" if dtype == np.float64 else "<f", z, 24)[0]
    mean = struct.unpack_from("<d" if dtype == np.float64 else "<f", z, 32)[0]
    s0, s1, s2 = struct.unpack_from("<III", z, 40)
    off = 56
    streams = []
    for sz in (s0, s1, s2):
        streams.append(zlib.decompress(bytes(z[off:off + sz])))
        off += sz
    q = np.frombuffer(bytes(z[off:off + 64 * np.dtype(dtype).itemsize]), dtype=dtype) if qt else None
    return dict(dt=dt, n=n, eb=eb, cnt=cnt, sf=sf, mean=mean, sizes=(s0, s1, s2), streams=streams, q=q,
                bindex_count=struct.unpack_from("<I", z, 52)[0] if qt else None)


def _feq(a, b):
    """Equal, or both NaN (the header of an array with a NaN in it: DESIGN.md section 4 row 7)."""
    return a == b or (a != a and b != b)


def _poison(x, kind):
    """The non-finite kinds of the drop-in's tests, on an array of any magnitude (tests/nonfinite.py has the bit patterns).
    The drop-in keeps util.c's first-element rule: a NaN x[0] makes max, sf and the whole result NaN."""
    n, dt = x.size, x.dtype
    p = (n // 2) // 64 * 64 + 4
    if kind == "qnan_one":
        NF.put_bits(x, p + 1, NF._QNAN[dt])
    elif kind == "snan_after_max":                          # the array's largest |x|, signalling NaNs behind it in its block
        x[p] = -10.0 * float(np.abs(x).max())
        NF.put_bits(x, np.array([p + 1, p + 2, p + 3, p + 16, p + 59]), NF._SNAN[dt])
    elif kind == "nan_first":
        NF.put_bits(x, 0, NF._QNAN[dt])
    elif kind == "nans_behind_finite_first":                # x[0] finite, everything else NaN: max = min = |x[0]|
        NF.put_bits(x, np.arange(1, n), NF._QNAN[dt])
    elif kind == "pos_inf":
        x[p + 1] = np.inf
    else:
        raise KeyError(kind)
    return x


NONFINITE = ["qnan_one", "snan_after_max", "nan_first", "nans_behind_finite_first", "pos_inf"]


@pytest.fixture(params=[0, 8, "gpu", "gpu_device_inflate"], ids=["zlib_ref_3threads", "zlib_chunked_8threads", "deflate_on_gpu", "deflate_and_inflate_on_gpu"])
def zthreads(request):
    """0: the reference's tail (three single-shot deflates); 8: chunked deflate (pdeflate.c); "gpu": the entropy stage
    on the device (DCTZ_ZLIB_GPU=1, dctzhip_deflate) -- the container is parsed with zlib's inflate in every case."""
    if request.param in ("gpu", "gpu_device_inflate"):
        os.environ["DCTZ_ZLIB_GPU"] = "1"
        if request.param == "gpu_device_inflate":          # the reader's indexed path through dctzhip_inflate instead of host threads
            os.environ["DCTZ_INFLATE_GPU"] = "1"
    elif request.param:
        os.environ["DCTZ_ZLIB_THREADS"] = str(request.param)
        os.environ["DCTZ_ZLIB_CHUNK"] = "65536"
    yield request.param
    os.environ.pop("DCTZ_ZLIB_THREADS", None)
    os.environ.pop("DCTZ_ZLIB_CHUNK", None)
    os.environ.pop("DCTZ_ZLIB_GPU", None)
    os.environ.pop("DCTZ_INFLATE_GPU", None)


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("case", ["c1", "ragged_f32", "ragged_f64_rem", "qnan_one"])
def test_dropin_compress_decompress(mode, case, zthreads):
    lib = _lib(mode)
    qt = mode == "qt"
    bad = None
    if case == "c1":
        x = W.c1(); eb = 1e-3
    elif case == "ragged_f32":
        x = W.ragged(64 * 700 + 17, np.float32, scale=37.0); eb = 1e-4
    elif case == "qnan_one":                              # one NaN costs one block
        x, bad = NF.make("qnan_one", 64 * 700 + 17, np.float64); eb = 1e-3
    else:
        x = W.ragged(37024, np.float64, scale=410.0); eb = 1e-3
    n = x.size
    orig = x.copy()
    zbuf = np.zeros(n * x.itemsize + 4096, np.uint8)     # dctz-test.c:143: N*type_size bytes
    rec = np.zeros(n, x.dtype)
    var, var_z, var_r = _tvar(x), TVar(), _tvar(rec)
    var_z.datatype = var.datatype
    var_z.buf.d = zbuf.ctypes.data_as(C.POINTER(C.c_double))
    out_size = C.c_size_t(0)
    assert lib.dctz_compress(C.byref(var), n, C.byref(out_size), C.byref(var_z), eb) == 1

    c = O.compress(orig, eb, O.QT if qt else O.EC, O.FAST)
    h = _parse(zbuf[:out_size.value], x.dtype, qt)
    assert (h["dt"], h["n"], h["eb"], h["cnt"]) == (var.datatype, n, eb, c.cnt)
    assert h["sf"] == c.sf
    assert _feq(h["mean"], x.dtype.type(c.mean))          # serial-order mean: bit-exact
    assert h["streams"][0] == c.bin_index.tobytes()
    # (same_with_nans: bit-identical, but for the payload of a NaN where the oracle has a NaN -- nowhere in clean data)
    assert NF.same_with_nans(np.frombuffer(h["streams"][1], np.float32), c.dc)
    assert NF.same_with_nans(np.frombuffer(h["streams"][2], np.float32), c.ac_exact)
    if qt:
        assert h["bindex_count"] == n and NF.same_with_nans(h["q"], c.qtable)
    assert NF.same_with_nans(x, c.scaled), "caller's buffer must hold x/sf"
    if bad is None:
        assert not np.isnan(c.dc).any() and not np.isnan(c.scaled).any()
    body = 56 + sum(h["sizes"]) + (64 * x.itemsize if qt else 0)
    if zthreads in ("gpu", "gpu_device_inflate"):          # "DZIX" chunk index behind the container (include/dctz.h)
        nblk = (n + 63) // 64
        nch = [(b + 16383) // 16384 for b in (n, 4 * nblk, 4 * c.cnt)]
        assert out_size.value == body + ((20 + 2 * sum(nch) + 3) & ~3)
        magic, chunk, n0, n1, n2 = struct.unpack_from("<IIIII", bytes(zbuf[body:body + 20]))
        assert (magic, chunk, [n0, n1, n2]) == (0x58495A44, 16384, nch)
        sizes = np.frombuffer(bytes(zbuf[body + 20:body + 20 + 2 * sum(nch)]), dtype=np.uint16)
        assert [int(sizes[:n0].sum()) + 8, int(sizes[n0:n0 + n1].sum()) + 8, int(sizes[n0 + n1:].sum()) + 8] == list(h["sizes"])
        assert all(bytes(zbuf[o:o + 2]) == b"\x78\x5e" for o in (56, 56 + h["sizes"][0], 56 + h["sizes"][0] + h["sizes"][1]))
    else:
        assert out_size.value == body
    if case == "c1" and mode == "ec" and zthreads == 0 and zlib.ZLIB_VERSION.startswith("1.2.11"):
        assert out_size.value == 3763394                   # survey known answer (zlib 1.2.11)

    if bad is not None:                                    # the container of an array with a NaN is a well-formed one
        lib.dctz_check_container.restype = C.c_int
        lib.dctz_check_container.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
        assert lib.dctz_check_container(zbuf.ctypes.data_as(C.c_void_p), out_size.value, n, 1) == 0
    assert lib.dctz_decompress(C.byref(var_z), C.byref(var_r)) == 1
    assert NF.same_with_nans(rec, O.decompress(c, O.FAST))
    if bad is None:
        assert not np.isnan(rec).any()
    else:                                                  # ... and decodes to NaN on exactly one block
        want = np.zeros(n, bool)
        want[64 * bad[0]:64 * bad[0] + 64] = True
        assert bad.size == 1 and np.array_equal(np.isnan(rec), want)
    if case == "c1" and mode == "ec":
        p = O.psnr((orig / c.sf) * c.sf, rec)
        assert abs(p["psnr"] - 96.383701092386) < 1e-6 and abs(p["maxdiff"] - 9.232739551845448e-05) < 1e-10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_tail_knobs(dtype):
    """DCTZ_ZLIB_GPU=1 with its two side knobs: DCTZ_SCALE_HOST=0 (x / sf written back by the GPU instead of host
    threads) gives the same container and the same caller's buffer; DCTZ_FAST_MEAN=1 changes nothing but the header's
    mean, which then is the tree-order sum / N (close to, not bit-identical with, the reference's serial sum)."""
    lib = _lib("ec")
    x0 = W.ragged(64 * 5000 + 21, dtype, scale=410.0)
    n = x0.size
    c = O.compress(x0, 1e-3, O.EC, O.FAST)

    def run(env):
        for k in ("DCTZ_ZLIB_GPU", "DCTZ_SCALE_HOST", "DCTZ_FAST_MEAN"):
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            x = x0.copy()
            zbuf = np.zeros(n * x.itemsize + 65536, np.uint8)
            var, var_z = _tvar(x), TVar()
            var_z.datatype = var.datatype
            var_z.buf.d = zbuf.ctypes.data_as(C.POINTER(C.c_double))
            out_size = C.c_size_t(0)
            assert lib.dctz_compress(C.byref(var), n, C.byref(out_size), C.byref(var_z), 1e-3) == 1
            return bytes(zbuf[:out_size.value]), x
        finally:
            for k in env:
                os.environ.pop(k, None)

    z_host_scale, x_a = run({"DCTZ_ZLIB_GPU": "1"})
    z_gpu_scale, x_b = run({"DCTZ_ZLIB_GPU": "1", "DCTZ_SCALE_HOST": "0"})
    z_fast, x_c = run({"DCTZ_ZLIB_GPU": "1", "DCTZ_FAST_MEAN": "1"})
    assert z_host_scale == z_gpu_scale
    for x in (x_a, x_b, x_c):
        assert np.array_equal(x.view(np.uint8), c.scaled.view(np.uint8))
    assert z_fast[:32] == z_host_scale[:32] and z_fast[40:] == z_host_scale[40:]
    w = np.dtype(dtype).itemsize
    m_ref = np.frombuffer(z_host_scale[32:32 + w], dtype)[0]
    m_fast = np.frombuffer(z_fast[32:32 + w], dtype)[0]
    assert m_ref == dtype(c.mean)
    assert abs(float(m_fast) - float(m_ref)) <= 1e-5 * float(np.abs(x0).max())


def test_dct_h_per_block_api():
    """dct_init / dct_fftw / ifft_idct / dct_finish as dct-test.c:81-89, 144-152 drives them."""
    lib = _lib("ec")
    x = W.ragged(64 * 3 + 40, np.float64)
    fwd = np.zeros_like(x); back = np.zeros_like(x)
    lib.dct_init(64)
    for b in range(4):
        l = min(64, x.size - 64 * b)
        if l != 64:
            lib.dct_finish(); lib.dct_init(l)
        lib.dct_fftw(x[64 * b:].ctypes.data_as(C.c_void_p), fwd[64 * b:].ctypes.data_as(C.c_void_p), l, 4)
    lib.dct_finish()
    for b in range(4):
        l = min(64, x.size - 64 * b)
        lib.ifft_idct(l, fwd[64 * b:].ctypes.data_as(C.c_void_p), back[64 * b:].ctypes.data_as(C.c_void_p))
    lib.idct_finish()
    ref = np.concatenate([O.dct_fwd(x[64 * b:64 * b + 64], O.FAST) for b in range(4)])
    assert np.array_equal(fwd.view(np.uint8), ref.view(np.uint8))
    assert np.abs(back - x).max() < 1e-13


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_per_block_calls_are_the_batched_kernels_bit_for_bit(dtype):
    """dct_fftw / ifft_idct run the product's lane flow on the HOST (dct_host.cpp: no PCIe round trip per 64 elements);
    the same blocks through dctz_dct_blocks -- the GPU kernels k_dct_blocks / k_dct_rem -- must be the same bytes, for
    every block length the codec can meet (1 .. 64), forward and inverse."""
    lib = _lib("ec")
    f = "" if dtype == np.float64 else "_f"
    fwd, inv, batched = getattr(lib, "dct_fftw" + f), getattr(lib, "ifft_idct" + f), getattr(lib, "dctz_dct_blocks" + f)
    getattr(lib, "dct_init" + f)(64)
    for l in range(1, 65):
        x = W.ragged(64 * 2 + l, dtype, scale=11.0)[-l:].copy()
        a, b, g = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        fwd(x.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), l, 1)
        batched(x.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), C.c_size_t(l), 0)
        assert np.array_equal(a.view(np.uint8), g.view(np.uint8)), f"forward, l={l}"
        inv(l, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        batched(a.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), C.c_size_t(l), 1)
        assert np.array_equal(b.view(np.uint8), g.view(np.uint8)), f"inverse, l={l}"
    getattr(lib, "dct_finish" + f)()


def test_dct_test_style_loop_is_not_a_pcie_round_trip_per_block():
    """dct-test.c:81-152's loop -- one call per 64-element block -- built in C against the drop-in: round 3 paid an H2D copy,
    a launch and a D2H copy per call (about 50 us per block); the reference's own FFTW path takes about 1 us."""
    import subprocess
    root = os.path.dirname(LIBDIR.rstrip("/")).rsplit("/dctz_amd", 1)[0]
    exe = os.path.join(root, "tests", "c", "dct_loop")
    lib_dir = LIBDIR
    subprocess.check_call(["gcc", "-O2", "-o", exe, os.path.join(root, "tests", "c", "dct_loop.c"), "-L" + lib_dir, "-ldctz-ec",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    out = subprocess.run([exe, "16384"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-800:]
    f_ns, i_ns, worst = (float(v) for v in out.stdout.split()[-3:])
    assert f_ns < 4000 and i_ns < 4000, out.stdout            # (measured: well under a microsecond each; the reference: about 1 us)
    assert worst < 1e-12


_PD_CASES = [(m, d, k) for k in [None] + NONFINITE for m in ("ec", "qt") for d in (np.float64, np.float32)]


@pytest.mark.parametrize("mode,dtype,kind", _PD_CASES,
                         ids=[f"{np.dtype(d).name}-{m}" + (f"-{k}" if k else "") for m, d, k in _PD_CASES])
def test_pipelined_decompress_is_the_serial_one(mode, dtype, kind, monkeypatch):
    """dctz_decompress of an indexed container works group by group (inflate of the groups ahead, H2D, kernels and D2H of
    finished groups overlapping): the reconstruction must be the bytes of the serial path and of the oracle -- here with
    a small group (DCTZ_PIPE_GROUP) so that an array of a few MB is six groups, a remainder block in the last one, and
    exceptions spread unevenly over the groups."""
    lib = _lib(mode)
    qt = mode == "qt"
    n = (1 << 18) * 5 + 64 * 1000 + 37
    x = W.ragged(n, dtype, scale=37.0)
    x[: 1 << 18] += (np.random.default_rng(3).standard_normal(1 << 18) * 3.0).astype(dtype)   # a noisy first group: most of AC_exact
    if kind:                                              # NaN / Inf kinds: NaN where the oracle's is, else the same bits
        _poison(x, kind)
    orig = x.copy()
    eb = 1e-3
    monkeypatch.setenv("DCTZ_ZLIB_GPU", "1")
    zbuf = np.zeros(n * x.itemsize + 4096, np.uint8)
    var, var_z = _tvar(x), TVar()
    var_z.datatype = var.datatype
    var_z.buf.d = zbuf.ctypes.data_as(C.POINTER(C.c_double))
    out_size = C.c_size_t(0)
    assert lib.dctz_compress(C.byref(var), n, C.byref(out_size), C.byref(var_z), eb) == 1
    ref = O.decompress(O.compress(orig, eb, O.QT if qt else O.EC, O.FAST), O.FAST)
    assert bool(np.isnan(ref).any()) == bool(kind)
    recs = {}
    for name, env in (("pipelined", {"DCTZ_PIPE_GROUP": str(1 << 18)}), ("serial", {"DCTZ_PIPELINE": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rec = np.zeros(n, dtype)
        var_r = _tvar(rec)
        assert lib.dctz_decompress(C.byref(var_z), C.byref(var_r)) == 1
        recs[name] = rec
        for k in env:
            monkeypatch.delenv(k)
    assert np.array_equal(recs["pipelined"].view(np.uint8), recs["serial"].view(np.uint8))
    assert NF.same_with_nans(recs["pipelined"], ref)
    # a damaged chunk in the middle: the pipelined reader notices and hands the container to the one-stream inflate,
    # which treats damage the way the reference's reader does (no crash, the call returns)
    monkeypatch.setenv("DCTZ_PIPE_GROUP", str(1 << 18))
    bad = zbuf.copy()
    bad[56 + 5000] ^= 0x40
    var_b = TVar()
    var_b.datatype = var.datatype
    var_b.buf.d = bad.ctypes.data_as(C.POINTER(C.c_double))
    rec = np.zeros(n, dtype)
    var_r = _tvar(rec)
    assert lib.dctz_decompress(C.byref(var_b), C.byref(var_r)) == 1


@pytest.mark.parametrize("kind", ["ragged", "flat", "short_last_group"] + NONFINITE)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pipelined_compress_is_the_serial_one(dtype, kind, monkeypatch):
    """dctz_compress of a large array with the entropy stage on the device works group by group (H2D of the groups ahead,
    max|x| on host threads, kernels + deflate + D2H of the groups that have landed, the in-place x /= sf following the
    copy): the container must be the serial path's byte for byte -- but for the header's tree-order `mean` -- and the
    caller's array the same x / sf.  A small group (DCTZ_PIPE_GROUP) makes an array of a few MB six groups with a
    remainder block in the last; the array's largest value sits in the last group (the scaling factor is the ARRAY's)."""
    lib = _lib("ec")
    n = (1 << 18) * 5 + 64 * 1000 + 37
    if kind == "short_last_group":                        # the last group is nothing but the array's short last block
        n = (1 << 18) * 4 + 37
    if kind == "flat":                                    # nothing stored exactly anywhere: AC_exact is the empty stream
        x = np.full(n, 42.5, dtype)
    else:
        x = W.ragged(n, dtype, scale=37.0)
        x[: 1 << 18] += (np.random.default_rng(3).standard_normal(1 << 18) * 3.0).astype(dtype)
        x[n - 70] = 5432.0
    if kind in NONFINITE:
        # NaN / Inf kinds.  The host's max|x| loops (mm_range_avx2 / mm_main) meet a NaN in every
        # worker's range in "nans_behind_finite_first" and signalling NaNs behind the maximum in "snan_after_max"; a NaN x[0]
        # sends the call to the serial path, which keeps util.c's rule (max = NaN, everything NaN).
        _poison(x, kind)
    orig = x.copy()
    eb = 1e-3
    monkeypatch.setenv("DCTZ_ZLIB_GPU", "1")
    monkeypatch.setenv("DCTZ_FAST_MEAN", "1")
    got = {}
    for name, env in (("pipelined", {"DCTZ_PIPE_GROUP": str(1 << 18)}), ("serial", {"DCTZ_PIPELINE": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        xin = orig.copy()
        zbuf = np.zeros(n * x.itemsize + 4096, np.uint8)
        var, var_z = _tvar(xin), TVar()
        var_z.datatype = var.datatype
        var_z.buf.d = zbuf.ctypes.data_as(C.POINTER(C.c_double))
        out_size = C.c_size_t(0)
        assert lib.dctz_compress(C.byref(var), n, C.byref(out_size), C.byref(var_z), eb) == 1
        got[name] = (zbuf[: out_size.value].copy(), xin, None)
        for k in env:
            monkeypatch.delenv(k)
    (zp, xp, _), (zs, xs, _) = got["pipelined"], got["serial"]
    assert zp.size == zs.size
    MEAN = slice(32, 40)                                   # struct header: mean at offset 32 (tests/test_abi_cpu.py)
    assert np.array_equal(np.delete(zp, np.r_[MEAN]), np.delete(zs, np.r_[MEAN]))
    mp = zp[MEAN].view(np.float64)[0] if dtype == np.float64 else zp[32:36].view(np.float32)[0]
    ms = zs[MEAN].view(np.float64)[0] if dtype == np.float64 else zs[32:36].view(np.float32)[0]
    c = O.compress(orig, eb, O.EC, O.FAST)                 # (util.c's first-element rule: the drop-in's)
    if np.isfinite(c.mean):
        assert abs(mp - ms) <= 1e-6 * max(1.0, abs(ms))
    else:
        assert kind in NONFINITE and not np.isfinite(mp) and not np.isfinite(ms)
    assert np.array_equal(xp.view(np.uint8), xs.view(np.uint8))
    hsf = zp[24:32].view(np.float64)[0] if dtype == np.float64 else zp[24:28].view(np.float32)[0]
    assert _feq(float(hsf), c.sf) and int(zp[16:20].view(np.uint32)[0]) == c.cnt
    if kind in NONFINITE:
        assert NF.same_with_nans(xp, c.scaled)
    else:
        sf = 10.0 ** (np.ceil(np.log10(np.abs(orig).max())) - 1)
        assert sf == c.sf and np.array_equal(xp, orig / dtype(sf))
    # ... and it decodes to the oracle's reconstruction
    ref = O.decompress(c, O.FAST)
    assert bool(np.isnan(ref).any()) == (kind in NONFINITE)
    var_z = TVar()
    var_z.datatype = _tvar(orig).datatype
    var_z.buf.d = zp.ctypes.data_as(C.POINTER(C.c_double))
    rec = np.zeros(n, dtype)
    var_r = _tvar(rec)
    assert lib.dctz_decompress(C.byref(var_z), C.byref(var_r)) == 1
    assert NF.same_with_nans(rec, ref)


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_host_buffer_batch_is_the_looped_calls(mode):
    """dctz_compress_batch / dctz_decompress_batch (additions to dctz.h): the list tests/test-dctz.sh loops over -- the six
    lengths of tests/list-msst19.txt under four bounds, plus one fp32 array -- in ONE call: every container byte for byte
    the one dctz_compress() writes for that array, every caller's array scaled in place the same way, every reconstruction
    the same bytes; and at least five times faster than the loop."""
    import time
    lib = _lib(mode)
    xs, ebs = [], []
    for i, n in enumerate(W.MSST19_LENGTHS):
        for eb in (1e-3, 1e-4, 1e-5, 1e-6):
            xs.append(W.c5_fp64(n, 3 + i)); ebs.append(eb)
    xs.append(W.ragged(64 * 900 + 21, np.float32, scale=5.0)); ebs.append(1e-4)
    k = len(xs)
    PT = C.POINTER(TVar)
    lib.dctz_compress_batch.restype = C.c_int
    lib.dctz_compress_batch.argtypes = [C.c_int, C.POINTER(PT), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(PT), C.POINTER(C.c_double)]
    lib.dctz_decompress_batch.restype = C.c_int
    lib.dctz_decompress_batch.argtypes = [C.c_int, C.POINTER(PT), C.POINTER(PT)]

    def looped():
        xa = [x.copy() for x in xs]
        zs = [np.zeros(x.nbytes + 4096, np.uint8) for x in xs]
        sizes = []
        t0 = time.perf_counter()
        for x, z, eb in zip(xa, zs, ebs):
            var, var_z = _tvar(x), TVar()
            var_z.datatype = var.datatype
            var_z.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
            out = C.c_size_t(0)
            assert lib.dctz_compress(C.byref(var), x.size, C.byref(out), C.byref(var_z), eb) == 1
            sizes.append(out.value)
        t1 = time.perf_counter()
        recs = [np.zeros_like(x) for x in xs]
        for x, z, r in zip(xs, zs, recs):
            var_z, var_r = TVar(), _tvar(r)
            var_z.datatype = 1 if x.dtype == np.float64 else 0
            var_z.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
            assert lib.dctz_decompress(C.byref(var_z), C.byref(var_r)) == 1
        t2 = time.perf_counter()
        return xa, zs, sizes, recs, t1 - t0, t2 - t1

    def batched():
        xa = [x.copy() for x in xs]
        zs = [np.zeros(x.nbytes + 4096, np.uint8) for x in xs]
        vars_, vars_z = [_tvar(x) for x in xa], []
        for x, z in zip(xa, zs):
            v = TVar()
            v.datatype = 1 if x.dtype == np.float64 else 0
            v.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
            vars_z.append(v)
        pv = (PT * k)(*[C.pointer(v) for v in vars_])
        pz = (PT * k)(*[C.pointer(v) for v in vars_z])
        ns = (C.c_int * k)(*[x.size for x in xs])
        outs = (C.c_size_t * k)()
        eb_a = (C.c_double * k)(*ebs)
        t0 = time.perf_counter()
        assert lib.dctz_compress_batch(k, pv, ns, outs, pz, eb_a) == 1
        t1 = time.perf_counter()
        recs = [np.zeros_like(x) for x in xs]
        vars_r = [_tvar(r) for r in recs]
        pr = (PT * k)(*[C.pointer(v) for v in vars_r])
        assert lib.dctz_decompress_batch(k, pz, pr) == 1
        t2 = time.perf_counter()
        return xa, zs, list(outs), recs, t1 - t0, t2 - t1

    looped(); batched()                                       # warm-up (context, device buffers, thread pools)
    la = looped()
    ba = batched()
    for i in range(k):
        assert la[2][i] == ba[2][i], i
        assert np.array_equal(la[1][i][:la[2][i]], ba[1][i][:ba[2][i]]), f"container {i}"
        assert np.array_equal(la[0][i].view(np.uint8), ba[0][i].view(np.uint8)), f"scaled array {i}"
        assert np.array_equal(la[3][i].view(np.uint8), ba[3][i].view(np.uint8)), f"reconstruction {i}"
    speed_c, speed_d = la[4] / ba[4], la[5] / ba[5]
    print(f"\nhost-buffer batch of {k} arrays ({mode}): compress {la[4] * 1e3:.2f} -> {ba[4] * 1e3:.2f} ms ({speed_c:.1f} x), "
          f"decompress {la[5] * 1e3:.2f} -> {ba[5] * 1e3:.2f} ms ({speed_d:.1f} x)")
    assert (la[4] + la[5]) / (ba[4] + ba[5]) >= 3.0          # (measured: see profiles/r04_host_batch.json; the bar here leaves room for a busy host)


def test_calc_data_stat_and_gen_bins():
    lib = _lib("ec")

    class U(C.Union):
        _fields_ = [("d", C.c_double), ("f", C.c_float)]

    class BStat(C.Structure):                               # dctz.h:68-94
        _fields_ = [("mean", U), ("min", U), ("max", U), ("range", U), ("sf", U)]
    for dtype in (np.float64, np.float32):
        x = W.ragged(100003, dtype, scale=512.0)
        bs = BStat()
        var = _tvar(x)
        lib.calc_data_stat(C.byref(var), C.byref(bs), x.size)
        st = O.stats(x)
        got = (bs.mean.d, bs.min.d, bs.max.d, bs.sf.d) if dtype == np.float64 else (bs.mean.f, bs.min.f, bs.max.f, bs.sf.f)
        assert got == tuple(dtype(v) for v in (st.mean, st.min, st.max, st.sf))
        # NaN / Inf: util.c's loop as it stands -- a NaN is passed over, except in x[0], where it stays
        for kind in NONFINITE:
            y = _poison(W.ragged(100003, dtype, scale=512.0), kind)
            bs = BStat()
            var = _tvar(y)
            lib.calc_data_stat(C.byref(var), C.byref(bs), y.size)
            st = O.stats(y)
            got = (bs.min.d, bs.max.d, bs.sf.d) if dtype == np.float64 else (bs.min.f, bs.max.f, bs.sf.f)
            want = tuple(dtype(v) for v in (st.min, st.max, st.sf))
            assert all(_feq(g, w) for g, w in zip(got, want)), (kind, got, want)
            m = bs.mean.d if dtype == np.float64 else bs.mean.f
            assert _feq(m, dtype(st.mean)) if np.isfinite(st.mean) else not np.isfinite(m), (kind, m, st.mean)
    bc = np.zeros(255)
    lib.gen_bins(C.c_double(0), C.c_double(0), bc.ctypes.data_as(C.c_void_p), 255, C.c_double(1e-3))
    assert np.array_equal(bc, O.gen_bins(1e-3, np.float64))


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_plain_c_caller_links_and_runs(mode, tmp_path):
    """A C program written against include/dctz.h only (the reference's calling
    convention) builds with gcc, links the drop-in library and round-trips."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / f"dropin_{mode}")
    flags = ["-DUSE_TRUNCATE"] + (["-DUSE_QTABLE"] if mode == "qt" else [])
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", os.path.join(root, "tests", "c", "dropin_roundtrip.c"),
                           "-I", os.path.join(root, "include"), "-L", LIBDIR, f"-ldctz-{mode}",
                           f"-Wl,-rpath,{LIBDIR}", "-lm", "-o", exe] + flags)
    for n, eb, f32 in ((100000, 1e-3, 0), (64 * 777 + 13, 1e-4, 1)):
        out = subprocess.check_output([exe, str(n), str(eb), str(f32)], env=dict(os.environ, DCTZ_QUIET="1"), text=True)
        line = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()
        psnr, maxerr = float(line[4]), float(line[5])
        assert int(line[1]) == n and float(line[3]) > 1.0
        assert psnr > 60.0 and maxerr <= 8.5 * eb * 10.0      # sf = 10 for |x| up to ~50
        # the zlib sections are fed / drained in pieces (sections beyond 4 GiB need it: avail_in / avail_out are 32-bit);
        # tiny pieces must give the very same container and reconstruction as one call per section
        out2 = subprocess.check_output([exe, str(n), str(eb), str(f32)], env=dict(os.environ, DCTZ_QUIET="1", DCTZ_ZLIB_PIECE="4099"), text=True)
        assert [l for l in out2.splitlines() if l.startswith("RESULT")] == [l for l in out.splitlines() if l.startswith("RESULT")]


def test_block_length_beyond_64_is_refused(tmp_path):
    """dct_fftw / ifft_idct take ANY dn in the reference (one length-dn plan, dct.c:55 / :115); the drop-in covers the
    codec's 1..64 and says so for anything longer instead of silently transforming 64-element pieces."""
    import subprocess, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "dn.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include "dctz.h"
        void dct_fftw(double *a, double *b, int dn, int nblk);
        int main(int argc, char **argv) {
          static double a[200], b[200];
          for (int i = 0; i < 200; i++) a[i] = i * 0.25;
          dct_fftw(a, b, argc > 1 ? 128 : 40, 1);
          puts(b[0] == b[0] ? "OK" : "NAN");
          return 0;
        }"""))
    exe = str(tmp_path / "dn")
    subprocess.check_call(["gcc", "-std=gnu99", str(src), "-I", os.path.join(root, "include"), "-L", LIBDIR, "-ldctz-ec",
                           f"-Wl,-rpath,{LIBDIR}", "-lm", "-o", exe, "-DUSE_TRUNCATE"])
    ok = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, DCTZ_QUIET="1"))
    assert ok.returncode == 0 and ok.stdout.startswith("OK")
    bad = subprocess.run([exe, "long"], capture_output=True, text=True, env=dict(os.environ, DCTZ_QUIET="1"))
    assert bad.returncode == 1 and "dn = 128" in bad.stderr


# ---- fuzz of the drop-in boundary: host buffers in, container out, both zlib tails ------------------
from hypothesis import HealthCheck, given, settings, strategies as st   # noqa: E402


@settings(max_examples=25, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(seed=st.integers(0, 2**31), n=st.integers(1, 300000), log_amp=st.floats(-4, 6), eb=st.sampled_from([1e-2, 1e-3, 1e-5]),
       mode=st.sampled_from(["ec", "qt"]), dtype=st.sampled_from([np.float64, np.float32]), zthreads=st.sampled_from([0, 5, -1]))
def test_dropin_fuzz(seed, n, log_amp, eb, mode, dtype, zthreads):
    os.environ.pop("DCTZ_ZLIB_GPU", None)
    if zthreads < 0:                                        # the entropy stage on the device
        os.environ["DCTZ_ZLIB_GPU"] = "1"
        os.environ.pop("DCTZ_ZLIB_THREADS", None)
    elif zthreads:
        os.environ["DCTZ_ZLIB_THREADS"] = str(zthreads)
        os.environ["DCTZ_ZLIB_CHUNK"] = "32768"
    else:
        os.environ.pop("DCTZ_ZLIB_THREADS", None)
    try:
        lib = _lib(mode)
        qt = mode == "qt"
        rng = np.random.default_rng(seed)
        t = np.arange(n) / 37.0
        amp = 10.0 ** log_amp
        x = (amp * (np.sin(t) + 0.2 * np.cos(3.1 * t)) + 0.01 * amp * rng.standard_normal(n)).astype(dtype)
        orig = x.copy()
        zbuf = np.zeros(n * x.itemsize + 8192, np.uint8)
        rec = np.zeros(n, dtype)
        var, var_z, var_r = _tvar(x), TVar(), _tvar(rec)
        var_z.datatype = var.datatype
        var_z.buf.d = zbuf.ctypes.data_as(C.POINTER(C.c_double))
        out_size = C.c_size_t(0)
        assert lib.dctz_compress(C.byref(var), n, C.byref(out_size), C.byref(var_z), eb) == 1
        c = O.compress(orig, eb, O.QT if qt else O.EC, O.FAST)
        h = _parse(zbuf[:out_size.value], dtype, qt)
        assert (h["n"], h["cnt"], h["sf"]) == (n, c.cnt, c.sf) and h["mean"] == dtype(c.mean)
        assert h["streams"] == [c.bin_index.tobytes(), c.dc.tobytes(), c.ac_exact.tobytes()]
        assert np.array_equal(x.view(np.uint8), c.scaled.view(np.uint8))
        lib.dctz_check_container.restype = C.c_int
        lib.dctz_check_container.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
        assert lib.dctz_check_container(zbuf.ctypes.data_as(C.c_void_p), out_size.value, n, 1) == 0
        assert lib.dctz_decompress(C.byref(var_z), C.byref(var_r)) == 1
        assert np.array_equal(rec.view(np.uint8), O.decompress(c, O.FAST).view(np.uint8))
    finally:
        os.environ.pop("DCTZ_ZLIB_THREADS", None)
        os.environ.pop("DCTZ_ZLIB_CHUNK", None)
        os.environ.pop("DCTZ_ZLIB_GPU", None)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_calc_psnr_on_the_gpu_agrees_with_its_host_loop(dtype, capfd):
    """calc_psnr (util.c:54-104) of the drop-in: arrays of 2^16 elements and more take the GPU reductions; the
    returned PSNR agrees with the host loop (DCTZ_PSNR_HOST=1, the reference's serial order) to 1e-12 relative and
    the 'Max relative error' line (util.c:95) is the same text."""
    lib = _lib("ec")
    lib.calc_psnr.argtypes = [C.POINTER(TVar), C.POINTER(TVar), C.c_int, C.c_double]
    rng = np.random.default_rng(77)
    n = (1 << 20) + 37
    x = (10 * np.sin(np.arange(n) / 311.0) + rng.normal(0, 0.3, n)).astype(dtype)
    r = (x.astype(np.float64) + rng.uniform(-1e-3, 1e-3, n)).astype(dtype)
    vx, vr = _tvar(x), _tvar(r)
    capfd.readouterr()
    os.environ.pop("DCTZ_PSNR_HOST", None)
    p_gpu = lib.calc_psnr(C.byref(vx), C.byref(vr), n, 1e-3)
    out_gpu = capfd.readouterr().out
    os.environ["DCTZ_PSNR_HOST"] = "1"
    try:
        p_host = lib.calc_psnr(C.byref(vx), C.byref(vr), n, 1e-3)
    finally:
        os.environ.pop("DCTZ_PSNR_HOST", None)
    out_host = capfd.readouterr().out
    assert abs(p_gpu - p_host) <= 1e-12 * abs(p_host)
    assert "Max relative error" in out_gpu and out_gpu == out_host
    # and against numpy in the data type
    e = x - r
    want = 20 * np.log10((float(x.max()) - float(x.min())) / np.sqrt(float(np.sum((e * e).astype(np.float64))) / n))
    assert abs(p_gpu - want) <= 1e-9 * abs(want)
