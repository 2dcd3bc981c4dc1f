"""The quantiser's launch constants of dctz_amd/csrc/dctz_quant_host.h (what every compress and decode path fills its parameter
block from), printed on the CPU by tests/c/quant_host_test.cpp -- built as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer -- and compared BIT FOR BIT with the numpy restatement of tests/bin_edge_cases.py (consts, classify,
classify_sf, the windows), which never calls the library."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import bin_edge_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ((np.float32, "f32"), (np.float64, "f64"))
FASTDIVS = (0, 1, 2)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quant_host") / "quant_host_test")
    # (-Wno-unknown-pragmas: dctz_tables.h, where scaling_factor lives, includes the lane headers and their unroll pragmas)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dctz_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "quant_host_test.cpp")])

    def run(requests):
        r = subprocess.run([exe] + list(requests), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return [ln.split() for ln in lines]
    return run


def hexd(v):
    return struct.pack(">d", float(v)).hex()


def hexbits(v, dtype):
    """The bit pattern of v in dtype, as the program prints it."""
    dtype = np.dtype(dtype)
    return format(int(np.asarray(v, dtype=dtype).reshape(1).view(np.uint64 if dtype == np.float64 else np.uint32)[0]), "x")


def sweep(dtype):
    """eb = m * 10^k over the decades that cross both edges of the divisor window of the bin width 2 eb: 2^+-30 ~ 1e+-9 (fp32),
    2^+-250 ~ 1.8e+-75 (fp64).  fp64: three decades past each edge.  fp32: every decade a float has, 1e-46 .. 1e38 -- below
    2^-126 a bound rounded to float is subnormal and has lost bits, and only there does decode's T(T(eb) * 2) differ from
    T(eb * 2): on 17 bounds of this sweep, 7e-46 .. 1e-38, which is where inv_quant without the inner cast fails this test.
    (A double is not rounded on the way in, so no fp64 bound can tell the two apart.)"""
    klo, khi = (-79, 79) if np.dtype(dtype) == np.float64 else (-46, 38)
    return [float(f"{m}e{k}") for k in range(klo, khi + 1) for m in (1, 1.25, 2.5, 3, 7)]


def bounds(dtype):
    case_ebs = sorted({c.eb for c in B.CASES if c.dtype == np.dtype(dtype)})
    return case_ebs + sweep(dtype)


def test_forward_and_inverse_constants(program):
    """fwd_quant against consts / classify; inv_quant against T(T(eb) * 2 * 1.0), T(eb * 255), T(-eb * 255)."""
    for dtype, tag in DTYPES:
        T = np.dtype(dtype).type
        ebs = bounds(dtype)
        for c in B.CASES:
            assert c.dtype != np.dtype(dtype) or c.eb in ebs
        census = {fd: {0: 0, 1: 0, 3: 0} for fd in FASTDIVS}
        keys = [(eb, fd) for eb in ebs for fd in FASTDIVS]
        got = program([f"q:{tag}:{hexd(eb)}:{fd}" for eb, fd in keys])
        for (eb, fd), g in zip(keys, got):
            with np.errstate(over="ignore", invalid="ignore"):
                bw, rmin, rmax = B.consts(eb, dtype)
                cls = B.classify(eb, dtype, fd)
                inv = (T(T(eb) * 2 * 1.0), T(-eb * 255), T(eb * 255))
            census[fd][cls] += 1
            want = [hexbits(bw, dtype), hexbits(rmin, dtype), hexbits(rmax, dtype), str(cls)] + [hexbits(v, dtype) for v in inv]
            assert g == want, (tag, eb, fd, g, want)
        # every class was met, at the setting that can give all three and at the ones that cannot
        assert all(census[2][k] >= 3 for k in (0, 1, 3)), (tag, census)
        assert census[1][0] >= 3 and census[1][1] >= 3 and census[1][3] == 0, (tag, census)
        assert census[0][0] == len(ebs), (tag, census)


def _edge_values(dtype):
    """Statistics: zero, subnormal, inf, NaN, ordinary values, and both sides of every window edge (value window 2^+-63 /
    2^+-500, and the values whose scaling factor crosses the divisor window 2^+-30 / 2^+-250)."""
    T = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    tiny = np.finfo(dtype).tiny
    vals = [T(0), T(tiny) / T(4), T(tiny), T(np.inf), T(np.nan), T(0.37), T(1), T(5), T(99.5), T(100), T(np.finfo(dtype).max)]
    for e in ((-500, 500, -250, 250) if f64 else (-63, 63, -30, 30)):
        p = T(2.0) ** T(e)
        vals += [np.nextafter(p, T(0)), p, np.nextafter(p, T(np.inf)), p * T(10), p * T(100), p / T(10)]
    return vals


def test_fast_sf_level(program):
    for dtype, tag in DTYPES:
        vals = _edge_values(dtype)
        keys = [(mx, mn, fd) for mx in vals for mn in vals if not mn > mx for fd in FASTDIVS]
        got = program([f"l:{tag}:{hexd(mx)}:{hexd(mn)}:{fd}" for mx, mn, fd in keys])
        census = {0: 0, 1: 0, 2: 0}
        for (mx, mn, fd), g in zip(keys, got):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                want = B.classify_sf(np.array([mx, mn], dtype=dtype), dtype, fd)
            census[want] += fd == 2
            # placeholder statistics (the device chooses sf): never level 2
            assert g == [str(want), str(min(want, 1))], (tag, mx, mn, fd, g, want)
        assert all(v >= 3 for v in census.values()), (tag, census)
        # the two sides of the value window's lower edge, with a scaling factor FastDiv may take
        T = np.dtype(dtype).type
        lo = T(2.0) ** T(-500 if np.dtype(dtype) == np.float64 else -63)
        inside, outside = program([f"l:{tag}:{hexd(1.0)}:{hexd(lo)}:2", f"l:{tag}:{hexd(1.0)}:{hexd(np.nextafter(lo, T(0)))}:2"])
        assert inside[0] == "2" and outside[0] == "1"


def _sf(mx, dtype):
    return O.stats(np.array([mx], dtype=dtype)).sf


def test_device_sf_verdict(program):
    for dtype, tag in DTYPES:
        T = np.dtype(dtype).type
        lo = T(2.0) ** T(-500 if np.dtype(dtype) == np.float64 else -63)
        out_of_window = float(np.nextafter(lo, T(0)))
        for mx in (T(0.5), T(1), T(37.25), T(100), T(100.5), T(3e-7), T(8.1e9), T(0)):
            sf = _sf(mx, dtype)
            rows = [(sf, 0, 1), (sf, 1, 1), (sf, 2, 1),                          # the host's own value: stands at every level
                    (sf * 10, 1, 0), (sf / 10, 1, 0), (float("nan"), 1, 0)]       # the neighbouring decades, a NaN
            mn = float(mx) / 2 if mx else 0.0
            got = program([f"v:{tag}:{hexd(mx)}:{hexd(mn)}:{hexd(s)}:{fast}" for s, fast, _ in rows])
            for (s, fast, want), g in zip(rows, got):
                if mx == 0 and fast == 2:
                    want = 0                                                    # (min = max = 0 is outside the value window)
                assert g == [str(want), hexbits(sf, np.float64)], (tag, mx, s, fast, g)
            # level 2 needs min and max inside the value window; levels 0 and 1 do not ask
            if mx:
                got = program([f"v:{tag}:{hexd(mx)}:{hexd(out_of_window)}:{hexd(sf)}:{fast}" for fast in (2, 1, 0)])
                assert [g[0] for g in got] == ["0", "1", "1"], (tag, mx, got)
    # fp32 compares in float: the device reports its float widened, the host's powf result is compared after the same rounding
    sf32 = _sf(np.float32(0.5), np.float32)
    assert sf32 == float(np.float32(0.1)) and sf32 != 0.1
    got = program([f"v:f32:{hexd(0.5)}:{hexd(0.25)}:{hexd(0.1)}:1", f"v:f64:{hexd(0.5)}:{hexd(0.25)}:{hexd(sf32)}:1",
                   f"v:f64:{hexd(0.5)}:{hexd(0.25)}:{hexd(0.1)}:1"])
    assert [g[0] for g in got] == ["1", "0", "1"]
