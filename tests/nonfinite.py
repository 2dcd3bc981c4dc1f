"""Arrays with NaN / Inf in them, and the comparison rule for what the codec makes of them.

One place for the CPU tests of the oracle, the GPU tests of every compress / decode path and the drop-in's tests:
the kinds are built on W.ragged(n, dtype, scale=37.0) and the non-finite bit patterns go in through an integer view
(no arithmetic ever touches them on the way: a signalling NaN stays signalling).

The rule every comparison against the oracle uses (same_with_nans):
  * integer streams and header scalars are exact;
  * a floating-point stream is NaN exactly where the oracle's is NaN -- sign and payload of the NaN are free (x86 and
    the GPU propagate payloads differently) -- and bit-identical everywhere else.
So that "it was NaN anyway" cannot hide a wrong kernel, the kinds whose damage is CONTAINED come with the number of
poisoned blocks, and the tests assert FROM THE ORACLE ALONE that no more than that many DC entries and 64 times as many
reconstructed elements are NaN (contained_budget)."""
import numpy as np

from tests import workloads as W

KINDS = ["qnan_one", "snan_one", "snan_after_max", "neg_nan", "nan_last_short", "nan_first", "nan_tile", "nan_sprinkled",
         "all_nan", "pos_inf", "neg_inf", "inf_first"]
INF_KINDS = ("pos_inf", "neg_inf", "inf_first")
# kinds that cost the poisoned blocks and nothing else under the device ABI's rule (a NaN is passed over by the statistics)
CONTAINED = [k for k in KINDS if k not in INF_KINDS and k != "all_nan"]

_U = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}
_QNAN = {np.dtype(np.float64): 0x7ff8000000000000, np.dtype(np.float32): 0x7fc00000}
_SNAN = {np.dtype(np.float64): 0x7ff4000000000000, np.dtype(np.float32): 0x7fa00000}        # quiet bit clear, payload set
_NEGNAN = {np.dtype(np.float64): 0xfff8000000000123, np.dtype(np.float32): 0xffc00123}     # sign bit set, a payload
SPIKE = 4321.0                                                                            # two decades above ragged(scale=37)


def put_bits(x, idx, bits):
    x.view(_U[x.dtype])[idx] = bits


def is_snan(x):
    """True where x holds a signalling NaN (exponent all ones, quiet bit clear, payload non-zero)."""
    u = x.view(_U[x.dtype])
    quiet = np.uint64(1 << 51) if x.dtype == np.float64 else np.uint32(1 << 22)
    return np.isnan(x) & ((u & quiet) == 0)


def interior_block(n):
    return ((n + 63) // 64) // 2


def make(kind, n, dtype, base=None):
    """-> (x, blocks): the array and the sorted indices of the 64-element blocks that hold a non-finite value.
    base: the finite array to poison (default W.ragged(n, dtype, scale=37.0))."""
    dt = np.dtype(dtype)
    x = (W.ragged(n, dtype, scale=37.0) if base is None else np.array(base, dtype=dtype, copy=True)).reshape(-1)
    assert x.size == n and np.isfinite(x).all() and float(np.abs(x).max()) < 100.0
    nblk = (n + 63) // 64
    b = interior_block(n)
    at = min(64 * b + 5, n - 1)
    if kind == "qnan_one":
        put_bits(x, at, _QNAN[dt])
    elif kind == "snan_one":
        put_bits(x, at, _SNAN[dt])
    elif kind == "snan_after_max":
        # the array's largest |x| early in block b, signalling NaNs behind it in the SAME block (the next element of its
        # 16-byte vector included): whoever walks the block with a running maximum must still have SPIKE at the end
        lo = 64 * b
        pos = np.array([p for p in (lo + 5, lo + 6, lo + 7, lo + 20, lo + 40, lo + 63) if p < n], dtype=np.int64)
        assert pos.size, "the block must have room for the spike and a NaN behind it"
        x[lo + 4] = -SPIKE
        put_bits(x, pos, _SNAN[dt])
    elif kind == "neg_nan":
        put_bits(x, at, _NEGNAN[dt])
    elif kind == "nan_last_short":
        put_bits(x, n - 1, _QNAN[dt])                             # the last block (ragged when n % 64 != 0)
    elif kind == "nan_first":
        put_bits(x, 0, _QNAN[dt])
    elif kind == "nan_tile":
        t = ((nblk + 63) // 64) // 2                              # an interior 4096-element tile: every block of it
        blocks = np.arange(64 * t, min(64 * t + 64, nblk))
        pos = np.minimum(64 * blocks + (7 * blocks + 3) % 64, n - 1)
        put_bits(x, pos, _QNAN[dt])
    elif kind == "nan_sprinkled":
        m = np.random.default_rng(20261016 + n).random(n) < 1e-3
        m[min(7, n - 1)] = True
        put_bits(x, np.flatnonzero(m), _QNAN[dt])
    elif kind == "all_nan":
        put_bits(x, np.arange(n), _QNAN[dt])
    elif kind == "pos_inf":
        x[at] = np.inf
    elif kind == "neg_inf":
        x[at] = -np.inf
    elif kind == "inf_first":
        x[0] = np.inf
    else:
        raise KeyError(kind)
    if kind.startswith("snan"):
        assert is_snan(x).any()
    bad = np.unique(np.flatnonzero(~np.isfinite(x)) // 64)
    assert bad.size >= 1
    return x, bad


def nan_mask_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))


def same_with_nans(got, want):
    """NaN exactly where `want` is NaN (sign and payload free); every other element bit-identical."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    m = np.isnan(want)
    if not np.array_equal(np.isnan(got), m):
        return False
    u = _U[got.dtype]
    return np.array_equal(got.view(u)[~m], want.view(u)[~m])


def describe_mismatch(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    m, g = np.isnan(want), np.isnan(got)
    u = _U[got.dtype]
    bad = np.flatnonzero((m != g) | (~m & ~g & (got.view(u) != want.view(u))))
    return (f"{bad.size} mismatches, first at {bad[:6]}; NaN here/there {int(g.sum())}/{int(m.sum())}; "
            f"got {got[bad[:4]]} want {want[bad[:4]]}")


def contained_budget(c, recon, nbad):
    """From the oracle's own result: the poisoned blocks' DC entries and reconstructions are all that may be NaN."""
    assert int(np.isnan(c.dc).sum()) <= nbad
    assert not np.isnan(c.ac_exact).any()
    assert int(np.isnan(recon).sum()) <= 64 * nbad
