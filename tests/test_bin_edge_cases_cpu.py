"""The bin-edge inputs of tests/bin_edge_cases.py, checked on the CPU from the oracle alone (no GPU): that every case holds
the coefficients it claims, that the numpy restatement of the host's predicates agrees with a direct enumeration, and --
the negative control -- that the data separates a right kernel from the subtly wrong one: bin_value restated WITHOUT the range
test differs from the oracle's bin ids at exactly the strip coefficients, the restatement WITH it nowhere."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bin_edge_cases as B

DTYPES = [np.float32, np.float64]
# every bound the suite compresses with, and those of the module
SOME_BOUNDS = [1e-6, 1e-5, 1e-4, 1e-3, 2e-3, 5e-4, 3e-4, 1e-2, 1.7e-4, 3.7e-5, 7.4e-5, 0.5, 1.0]


@pytest.mark.parametrize("case", B.CASES, ids=repr)
def test_census(case):
    """Each claimed class holds at least NEED coefficients (counted from the oracle's coefficient tap)."""
    got = case.census()
    print(case.name, got)
    for k in case.claims:
        assert got[k] >= B.NEED, (case.name, k, got)
    if "strip" not in case.claims:
        assert got["strip"] == 0 and not B.strip(case.eb, case.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounds_are_what_they_are_chosen_for(dtype):
    b = B.BOUNDS[np.dtype(dtype)]
    assert B.classify(b["strip"], dtype) == 1 and B.strip(b["strip"], dtype) and B.strip_width(b["strip"], dtype) == 1
    assert B.classify(b["bit1"], dtype) == 3 and not B.strip(b["bit1"], dtype)
    if "plain" in b:
        assert B.classify(b["plain"], dtype) == 0 and b["plain"] >= 2.0 ** 29
    for eb in b.values():
        assert eb >= 1e-6                          # (the entry points refuse anything smaller)
        assert B.classify(eb, dtype, fastdiv=0) == 0 and B.classify(eb, dtype, fastdiv=1) <= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("eb", SOME_BOUNDS + [6e8])
def test_classify_against_enumeration(eb, dtype):
    """Bit 1 promises q >= 255 for EVERY item above range_max: the next 200 floats, one by one.  Where it is clear, range_max
    itself has q < 255, and the floats above it that still do are the strip -- strip() tells whether there are any."""
    _, _, rmax = B.consts(eb, dtype)
    q = B.quotient(B.above_max(eb, dtype, 200), eb, dtype)
    assert np.all(np.diff(q) >= 0)
    bits = B.classify(eb, dtype)
    width = int((q < 255).sum())
    if bits & 2:
        assert width == 0 and B.quotient(rmax, eb, dtype) >= 255
    elif bits & 1:
        assert B.quotient(rmax, eb, dtype) < 255
    assert B.strip(eb, dtype) == (width > 0) and B.strip_width(eb, dtype) == width
    assert np.all(q[width:] >= 255)                # the strip is the FIRST floats above range_max
    # bit 0: the frexp window on the bin width
    bw = float(B.consts(eb, dtype)[0])
    lo, hi = (2.0 ** -250, 2.0 ** 250) if np.dtype(dtype) == np.float64 else (2.0 ** -30, 2.0 ** 30)
    assert bool(bits & 1) == (lo <= bw < hi)


def test_fp32_default_bound_has_the_strip_and_fp64_1e6_has_none():
    assert B.classify(1e-3, np.float32) == 1 and B.strip_width(1e-3, np.float32) == 1
    assert B.classify(1e-6, np.float64) == 1 and B.strip_width(1e-6, np.float64) == 0
    for eb in (1e-2, 1e-4, 1e-5):
        assert B.classify(eb, np.float32) == 3 and B.classify(eb, np.float64) == 3


@pytest.mark.parametrize("case", [c for c in B.CASES if c.kind != "short"], ids=repr)
def test_negative_control(case):
    """The unsafe form differs from the oracle at exactly the strip coefficients (>= NEED of them where the case claims the
    strip, none elsewhere); the safe form equals the oracle everywhere."""
    (c,) = case.oracle(O.EC, True)
    assert not np.isnan(c.coef).any()
    safe = B.bin_ids(c.coef, case.eb, case.dtype, True)
    unsafe = B.bin_ids(c.coef, case.eb, case.dtype, False)
    assert np.array_equal(safe, c.bin_index)
    differs = unsafe != c.bin_index
    strip = B.strip_mask(c.coef, case.eb, case.dtype)
    assert np.array_equal(differs, strip)
    n = int(differs.sum())
    print(case.name, "unsafe differs at", n)
    if "strip" in case.claims:
        assert n >= B.NEED
        assert np.all(c.bin_index[strip] == 255) and np.all(unsafe[strip] == 253)
    else:
        assert n == 0


@pytest.mark.parametrize("case", B.select("short"), ids=repr)
def test_negative_control_short(case):
    """The same for the short last blocks (bin_short carries a range test of its own): over all arrays of the case."""
    n = 0
    for c in case.oracle(O.EC, True):
        safe = B.bin_ids(c.coef, case.eb, case.dtype, True)
        unsafe = B.bin_ids(c.coef, case.eb, case.dtype, False)
        assert np.array_equal(safe, c.bin_index)
        differs = unsafe != c.bin_index
        assert np.array_equal(differs, B.strip_mask(c.coef, case.eb, case.dtype))
        n += int(differs.sum())
    assert n >= B.NEED if "strip" in case.claims else n == 0


def test_sets_are_small_and_cover_the_sublists():
    for dtype in DTYPES:
        eb = B.BOUNDS[np.dtype(dtype)]["strip"]
        assert B.flat_set(eb, dtype).size <= 400_000 and B.flat_set(eb, dtype).size % 64 == 0
        for nd in (2, 3):
            assert B.tiled_set(eb, dtype, nd).size <= 71_000
        for l in B.SHORT_LS:
            assert all(x.size == 64 + l for x in B.short_set(eb, dtype, l))
    assert {j // 16 for j in B.JS} == set(range(4)) and {j // 8 for j in B.JS} == set(range(8))
    assert any(l % 2 for l in B.SHORT_LS) and any(l % 2 == 0 for l in B.SHORT_LS)


def test_scaled_sets_have_sf_100():
    for case in B.select("flat"):
        (c,) = case.oracle(O.EC, True)
        assert c.sf == (100.0 if "sf100" in case.name else 1.0)
