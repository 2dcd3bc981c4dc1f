"""Inputs whose coefficients land on the bin edges (tests/test_bin_edge_cases_cpu.py, tests/test_gpu_bin_edges.py; DESIGN.md
section 4, "Bin edges, what is pinned").

Whether a coefficient is binned or stored exactly is decided 63 times per block, and the kernels decide it in one of three
variants chosen at launch (FwdParams::fast_bw): bit 0 "the bin width is in FastDiv's divisor window", bit 1 "item > range_max
=> q >= 255 holds in T arithmetic, so bin_value<T, SAFE = false> may drop the reference's range test".  Where bit 1 is clear
the two forms differ on the coefficients just above range_max whose quotient still rounds below 255 (the STRIP: one ulp wide
for the bounds used here).  Smooth or random data never puts a coefficient there, so the arrays of this module are built to:

  a block is ONE basis function of its transform, x[n] = a sqrt(2/64) cos(pi (2n + 1) j / 128), so that coefficient j is `a`
  plus a few ulps of transform noise; `a` sweeps +-SWEEP ulps around range_max, range_min and one interior edge
  range_min + M bin_width; one more block of 5.0 makes sf = 1 (a set scaled by 100 has sf = 100: x / sf runs first).

The same with the separable bases of the 8 x 8 and 4 x 4 x 4 tiles, and with the l-point basis of a short last block.  What an
array really holds is COUNTED from the oracle's coefficient tap (census): a case claims classes, and each claimed class must
hold at least NEED coefficients -- a condition on the data, checked on the CPU, that keeps the GPU tests from passing vacuously.

classify / strip_width restate the host's predicates (dctz_quant_host.h: divisor_in_window and the bit-1 test of fwd_quant) in
numpy, never calling them (tests/test_quant_host_cpu.py compares the two bit for bit); bin_ids restates bin_value in its two forms for the negative control."""
import functools
import math

import numpy as np

from oracle import oracle as O

BLK = 64
NEED = 4                                # coefficients per claimed class
SWEEP = 32                              # ulps either side of a target
M_EDGE = 100                            # the interior edge: range_min + M_EDGE * bin_width
JS = (5, 12, 21, 26, 37, 44, 53, 62)    # one position in each of k_compress's sub-list ranges (4 x 16; QT on fp64: 8 x 8)
K_FLAT = 4 * (2 * SWEEP + 1)            # blocks per (target, position): four sweeps
CLASSES = ("strip", "at_max", "at_min", "below_min", "int_q")

# error bounds per element type (chosen from classify / strip_width; test_bin_edge_cases_cpu.py asserts what they are chosen for)
#   strip   bit 1 clear and nextafter(range_max) has q < 255: SAFE and unsafe binning differ there
#   bit1    bit 1 set: the kernels run without the range test
#   plain   (fp32) the bin width is outside FastDiv's divisor window: plain division, no knob needed
BOUNDS = {
    np.dtype(np.float32): {"strip": 1e-3, "bit1": 1e-2, "plain": 6e8},
    np.dtype(np.float64): {"strip": 1.7e-4, "bit1": 1e-2},
}


def consts(eb, dtype):
    """bin_width, range_min, range_max as every compress path computes them: in double, stored in T (dctz-comp-lib.c:271-281)."""
    T = np.dtype(dtype).type
    eb = float(eb)
    return T(eb * 2.0 * 1.0), T(-255 * (eb * 1.0)), T(255 * (eb * 1.0))


def _exp_in(v, lo, hi):
    v = float(v)
    if v != v or v == 0.0 or math.isinf(v):
        return False
    e = math.frexp(abs(v))[1] - 1
    return lo <= e < hi


def divisor_in_window(d, dtype):
    return _exp_in(d, -250, 250) if np.dtype(dtype) == np.float64 else _exp_in(d, -30, 30)


def value_in_window(v, dtype):
    return _exp_in(v, -500, 500) if np.dtype(dtype) == np.float64 else _exp_in(v, -63, 63)


def quotient(item, eb, dtype):
    """(item - range_min) / bin_width in T, the reference's expression (:377 / :402)."""
    bw, rmin, _ = consts(eb, dtype)
    item = np.asarray(item, dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((item - rmin) / bw).astype(dtype)


def classify(eb, dtype, fastdiv=2):
    """FwdParams::fast_bw as the host sets it (DCTZHIP_FASTDIV = fastdiv)."""
    bw, rmin, rmax = consts(eb, dtype)
    if not fastdiv or not divisor_in_window(bw, dtype):
        return 0
    T = np.dtype(dtype).type
    u = T(rmax - rmin)
    q = T(u / bw)
    return 3 if (fastdiv >= 2 and q >= T(255)) else 1


def classify_sf(x, dtype, fastdiv=2):
    """FwdParams::fast_sf for the array x (host and device rule alike): 0 plain division, 1 FastDiv with a window test per
    element, 2 without."""
    sf = O.stats(np.ascontiguousarray(x).reshape(-1)).sf
    a = np.abs(np.asarray(x, dtype=np.float64))
    if not fastdiv or not divisor_in_window(np.dtype(dtype).type(sf), dtype):
        return 0
    return 2 if (fastdiv >= 2 and value_in_window(a.min(), dtype) and value_in_window(a.max(), dtype)) else 1


def variant(x, eb, dtype, fastdiv=2):
    """dctzhip_debug_counter 20 as predicted: fast_sf | fast_bw << 8."""
    return classify_sf(x, dtype, fastdiv) | classify(eb, dtype, fastdiv) << 8


def above_max(eb, dtype, count=200):
    """The next `count` floats above range_max."""
    _, _, rmax = consts(eb, dtype)
    return step_ulps(rmax, np.arange(1, count + 1), dtype)


def strip_width(eb, dtype, count=200):
    """How many of the floats above range_max have q < 255 (they are the first ones: rounding is monotonic)."""
    return int((quotient(above_max(eb, dtype, count), eb, dtype) < 255).sum())


def strip(eb, dtype):
    _, _, rmax = consts(eb, dtype)
    T = np.dtype(dtype).type
    return bool(quotient(np.nextafter(rmax, T(np.inf)), eb, dtype) < 255)


def step_ulps(t, k, dtype):
    """t moved by k ulps (k an integer array) in value order; t far from zero."""
    dtype = np.dtype(dtype)
    it = np.int64 if dtype == np.float64 else np.int32
    bits = np.asarray(t, dtype=dtype).reshape(1).view(it)[0]
    k = np.asarray(k, dtype=np.int64)
    out = (np.int64(bits) + (k if t > 0 else -k)).astype(it)
    return out.view(dtype)


def targets(eb, dtype):
    bw, rmin, rmax = consts(eb, dtype)
    T = np.dtype(dtype).type
    return (rmax, rmin, T(rmin + T(M_EDGE) * bw))


def amplitudes(eb, dtype, per_target, sweep=SWEEP, which=(0, 1, 2)):
    """per_target amplitudes around each target of `which`, sweeping -sweep .. +sweep ulps over and over."""
    tg = targets(eb, dtype)
    k = np.arange(per_target) % (2 * sweep + 1) - sweep
    return np.concatenate([step_ulps(tg[w], k, dtype) for w in which])


def _basis(l, j):
    n = np.arange(l, dtype=np.float64)
    return math.sqrt((1.0 if j == 0 else 2.0) / l) * np.cos(math.pi * (2.0 * n + 1.0) * j / (2.0 * l))


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def flat_set(eb, dtype, scale=1.0):
    """A block of 5.0; for every position of JS and every target, K_FLAT blocks; the block of 5.0 again.  ~400k elements.
    (The first block is there for the speculative calls: their sample always holds the array's first 4 KiB, so the guess
    of sf is right and the pass with fused statistics is the one that stands.)"""
    dtype = np.dtype(dtype)
    blocks = [np.full((1, BLK), 5.0)]
    for j in JS:
        a = amplitudes(eb, dtype, K_FLAT).astype(np.float64)
        blocks.append(a[:, None] * _basis(BLK, j)[None, :])
    blocks.append(np.full((1, BLK), 5.0))
    return _ro((np.concatenate(blocks) * scale).astype(dtype).reshape(-1))


ND_POS = {2: ((0, 5), (3, 0), (2, 6), (7, 7)), 3: ((0, 0, 3), (1, 2, 0), (3, 3, 3), (2, 1, 2))}
ND_SHAPE = {2: (264, 264), 3: (40, 40, 44)}          # 1089 tiles of 8 x 8, 1100 tiles of 4 x 4 x 4: ~70k elements


@functools.lru_cache(maxsize=None)
def tiled_set(eb, dtype, ndim, scale=1.0):
    """The same with the separable basis of an 8 x 8 / 4 x 4 x 4 tile: tile t is a * b_p (x) b_q [(x) b_r]; the last tile is 5.0."""
    dtype = np.dtype(dtype)
    e = O.GEOM_EDGE[ndim]
    shape = ND_SHAPE[ndim]
    ntile = int(np.prod([d // e for d in shape]))
    pos = ND_POS[ndim]
    per = (ntile - 1) // (3 * len(pos))
    lin = np.full((ntile, BLK), 5.0)
    t = 0
    for p in pos:
        b = _basis(e, p[0])
        for c in p[1:]:
            b = np.multiply.outer(b, _basis(e, c))
        a = amplitudes(eb, dtype, per, sweep=8).astype(np.float64)
        lin[t:t + a.size] = a[:, None] * b.reshape(-1)[None, :]
        t += a.size
    return _ro(O.nd_scatter((lin * scale).astype(dtype).reshape(-1), shape))


SHORT_LS = (40, 27)                     # l even and l odd
SHORT_POS = 14                          # positions j per l, spread over 1 .. l - 1
SHORT_SWEEP = 4                         # ulps either side (the l-point transform's noise is 3 ulps at the most)


@functools.lru_cache(maxsize=None)
def short_set(eb, dtype, l):
    """Arrays of 64 + l elements, one per amplitude: a block of 5.0, then a short last block that is a times the l-point
    basis function j.  For each of SHORT_POS positions j, a sweeps +-SHORT_SWEEP ulps around +range_max and around range_min
    (252 arrays).  The noise of the l-point transform is a fixed function of (a, j), so it is the positions that vary it."""
    dtype = np.dtype(dtype)
    xs = []
    for j in np.unique(np.linspace(1, l - 1, SHORT_POS).astype(int)):
        a = amplitudes(eb, dtype, 2 * SHORT_SWEEP + 1, sweep=SHORT_SWEEP, which=(0, 1)).astype(np.float64)
        tail = a[:, None] * _basis(l, int(j))[None, :]
        xs.append(np.concatenate([np.full((a.size, BLK), 5.0), tail], axis=1).astype(dtype))
    return tuple(_ro(np.ascontiguousarray(v)) for v in np.concatenate(xs))


def census(coef, eb, dtype):
    """Counts over the AC coefficients `coef` (the oracle's tap, block after block): the five classes of CLASSES."""
    bw, rmin, rmax = consts(eb, dtype)
    T = np.dtype(dtype).type
    coef = np.asarray(coef, dtype=dtype).reshape(-1)
    ac = coef[np.arange(coef.size) % BLK != 0]
    q = quotient(ac, eb, dtype)
    inside = (ac > rmin) & (ac < rmax)
    return {
        "strip": int(((ac > rmax) & (q < 255)).sum()),
        "at_max": int((ac == rmax).sum()),
        "at_min": int((ac == rmin).sum()),
        "below_min": int((ac == np.nextafter(rmin, T(-np.inf))).sum()),
        "int_q": int((inside & (q == np.floor(q)) & (q > 0) & (q < 255)).sum()),
    }


def strip_mask(coef, eb, dtype):
    """The positions (of the whole array) whose AC coefficient lies in the strip."""
    _, _, rmax = consts(eb, dtype)
    coef = np.asarray(coef, dtype=dtype).reshape(-1)
    m = (coef > rmax) & (quotient(coef, eb, dtype) < 255)
    m[::BLK] = False
    return m


def bin_ids(coef, eb, dtype, safe):
    """bin_value<T, SAFE> (dctz_kernel_common.h) restated: f = floor(q), h = |254.5 - 2 f| - 0.5, the range test only where
    `safe`, saturated to a byte as the packing conversion does; a NaN gives 0; the DC position holds 255."""
    _, _, rmax = consts(eb, dtype)
    T = np.dtype(dtype).type
    coef = np.asarray(coef, dtype=dtype).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(quotient(coef, eb, dtype))
        h = (np.abs(T(254.5) - T(2) * f) - T(0.5)).astype(np.float32)
        if safe:
            h = np.where(np.abs(coef) > rmax, np.float32(255), h)
        b = np.where(h != h, 0, np.clip(h, 0, 255)).astype(np.uint8)
    b[::BLK] = 255
    return b


class Case:
    """One array (or, kind "short", one list of arrays) at one bound, with the classes it claims."""

    def __init__(self, name, kind, dtype, eb, claims, scale=1.0, ndim=0, l=0):
        self.name, self.kind, self.dtype, self.eb, self.claims = name, kind, np.dtype(dtype), float(eb), tuple(claims)
        self.scale, self.ndim, self.l = scale, ndim, l

    def __repr__(self):
        return self.name

    def arrays(self):
        if self.kind == "flat":
            return (flat_set(self.data_eb, self.dtype, self.scale),)
        if self.kind == "tiled":
            return (tiled_set(self.data_eb, self.dtype, self.ndim, self.scale),)
        return short_set(self.data_eb, self.dtype, self.l)

    @property
    def data_eb(self):
        """The bound whose edges the data is built around: the case's own, but the strip bound's for an out-of-window
        bound (every coefficient is binned then: the case is about the plain-division variant running at all)."""
        b = BOUNDS[self.dtype]
        return b["strip"] if self.eb == b.get("plain") else self.eb

    def oracle(self, mode=O.EC, want_coef=False):
        return _oracle(self, mode, want_coef)

    def census(self):
        tot = dict.fromkeys(CLASSES, 0)
        for c in self.oracle(O.EC, True):
            for k, v in census(c.coef, self.eb, self.dtype).items():
                tot[k] += v
        return tot


@functools.lru_cache(maxsize=None)
def _oracle(case, mode, want_coef):
    """O.compress / O.compress_nd (FAST) of every array of the case, computed once; never modified."""
    f = O.compress_nd if case.kind == "tiled" else O.compress
    return tuple(f(x, case.eb, mode, O.FAST, want_coef) for x in case.arrays())


def _cases():
    out = []
    everything = ("strip", "at_max", "at_min", "below_min", "int_q")
    no_strip = ("at_max", "at_min", "below_min", "int_q")
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        b = BOUNDS[np.dtype(dtype)]
        for scale, stag in ((1.0, "sf1"), (100.0, "sf100")):
            out.append(Case(f"flat-{tag}-strip-{stag}", "flat", dtype, b["strip"], everything, scale))
            out.append(Case(f"flat-{tag}-bit1-{stag}", "flat", dtype, b["bit1"], no_strip, scale))
        if "plain" in b:
            out.append(Case(f"flat-{tag}-plain-sf1", "flat", dtype, b["plain"], (), 1.0))
        for ndim in (2, 3):
            out.append(Case(f"tiled{ndim}d-{tag}-strip", "tiled", dtype, b["strip"], ("strip", "at_max", "at_min", "below_min"), ndim=ndim))
            out.append(Case(f"tiled{ndim}d-{tag}-bit1", "tiled", dtype, b["bit1"], ("at_max", "at_min", "below_min"), ndim=ndim))
        for l in SHORT_LS:
            out.append(Case(f"short{l}-{tag}-strip", "short", dtype, b["strip"], ("strip", "at_max", "at_min", "below_min"), l=l))
            out.append(Case(f"short{l}-{tag}-bit1", "short", dtype, b["bit1"], ("at_max", "at_min", "below_min"), l=l))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def select(kind=None, dtype=None, tag=None):
    return [c for c in CASES if (kind is None or c.kind == kind) and (dtype is None or c.dtype == np.dtype(dtype))
            and (tag is None or f"-{tag}" in c.name)]
