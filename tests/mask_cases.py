"""The missing-value layer restated in numpy (include/dctz_hip.h, "missing values"): the tests that make an element missing,
the mask words, the fill rule -- vectorised, no Python loop over elements -- and the case list the GPU tests share: sizes,
patterns of missing elements, rules, and the inputs built from them."""
import numpy as np

MISS_NAN, MISS_INF, MISS_VALUE, MISS_ABS_GE = 1, 2, 4, 8
BLOCK = 64

SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 64 * 777 + 45, 2 ** 18 + 29)


def _bits(dtype):
    return np.uint64 if np.dtype(dtype) == np.float64 else np.uint32


def is_missing(x, flags, value=0.0, limit=0.0):
    """Boolean array: the selected tests, made in x's own type."""
    T = x.dtype.type
    m = np.zeros(x.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if flags & MISS_NAN:
            m |= x != x
        if flags & MISS_INF:
            m |= np.abs(x) == np.inf
        if flags & MISS_VALUE:
            m |= x == T(value)
        if flags & MISS_ABS_GE:
            m |= np.abs(x) >= T(limit)
    return m


def mask_words(miss):
    """ceil(n / 64) uint64 words: bit i & 63 of word i >> 6 is set iff element i is missing; bits beyond n are 0."""
    n = miss.size
    words = -(-n // BLOCK)
    padded = np.zeros(words * BLOCK, bool)
    padded[:n] = miss
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def mask_bits(words, n):
    """The inverse: the first n bits of the words as a boolean array."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def fill(x, miss):
    """The filled array: a missing element takes the nearest valid element before it in its 64-element block, else the block's
    first valid element, else +0.0.  Values move as bit patterns, so every filled value is an exact copy."""
    n = x.size
    U = _bits(x.dtype)
    nb = -(-n // BLOCK)
    xb = np.zeros(nb * BLOCK, U)
    xb[:n] = x.view(U)
    valid = np.zeros(nb * BLOCK, bool)
    valid[:n] = ~miss
    xb, valid = xb.reshape(nb, BLOCK), valid.reshape(nb, BLOCK)
    j = np.arange(BLOCK)
    prev = np.maximum.accumulate(np.where(valid, j, -1), axis=1)      # index of the last valid element at or before j
    first = np.argmax(valid, axis=1)                                 # index of the first valid element (0 if there is none)
    src = np.where(prev >= 0, prev, first[:, None])
    got = np.take_along_axis(xb, src, axis=1)
    out = np.where(valid.any(axis=1)[:, None], got, U(0))
    return out.reshape(-1)[:n].copy().view(x.dtype)


def fill_loop(x, miss):
    """The same rule as a plain loop over blocks and elements (small arrays only: what pins fill())."""
    out = x.copy()
    ob = out.view(_bits(x.dtype))
    for b0 in range(0, x.size, BLOCK):
        b1 = min(b0 + BLOCK, x.size)
        valid = [i for i in range(b0, b1) if not miss[i]]
        for i in range(b0, b1):
            if miss[i]:
                before = [v for v in valid if v < i]
                ob[i] = ob[before[-1]] if before else ob[valid[0]] if valid else 0
    return out


# ---- patterns of missing elements: name -> boolean array of n ----
def _blobs(n, seed=5):
    i = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 6.28, 3)
    f = np.sin(i / 211.0 + ph[0]) + np.sin(i / 37.0 + ph[1]) + 0.5 * np.sin(i / 1013.0 + ph[2])
    return f > 0.75


def pattern(name, n):
    m = np.zeros(n, bool)
    last0 = (n - 1) // BLOCK * BLOCK                      # start of the last block (short or whole)
    if name == "none":
        pass
    elif name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[n - 1] = True
    elif name == "whole_block":                           # the second block where there is one, with valid blocks around it
        b0 = BLOCK if n > BLOCK else 0
        m[b0:b0 + BLOCK] = True
    elif name == "leading_gap":                           # every block starts with a gap of another length
        i = np.arange(n)
        m = (i % BLOCK) < (i // BLOCK * 7 % 61 + 1)
        if n > 1:
            m[min(n, BLOCK) - 1] = False
    elif name == "trailing_gap":
        i = np.arange(n)
        m = (i % BLOCK) >= BLOCK - (i // BLOCK * 5 % 59 + 1)
    elif name == "alternate":
        m[::2] = True
    elif name == "random30":
        m = np.random.default_rng(n).random(n) < 0.3
    elif name == "blobs":
        m = _blobs(n)
    elif name == "across_boundaries":                     # a gap over a block boundary and one over a 4096-element boundary
        for edge, w in ((BLOCK, 3), (4096, 70), (2 * 4096, 1)):
            if n > edge - w:
                m[max(edge - w, 0):min(edge + w, n)] = True
    elif name == "last_block_all":
        m[last0:] = True
    elif name == "last_block_leading":
        m[last0:last0 + max((n - last0) // 2, 1)] = True
    else:
        raise KeyError(name)
    return m


PATTERNS = ("none", "all", "first", "last", "whole_block", "leading_gap", "trailing_gap", "alternate", "random30", "blobs",
            "across_boundaries", "last_block_all", "last_block_leading")

# ---- rules: name -> (flags, value, limit) ----
RULES = {
    "nan": (MISS_NAN, 0.0, 0.0),
    "inf": (MISS_INF, 0.0, 0.0),
    "value": (MISS_VALUE, 1e36, 0.0),
    "value0": (MISS_VALUE, 0.0, 0.0),                    # -0.0 matches
    "abs_ge": (MISS_ABS_GE, 0.0, 1e30),
    "nan_inf_abs_ge": (MISS_NAN | MISS_INF | MISS_ABS_GE, 0.0, 1e30),
}


def _from_bits(dtype, *patterns):
    return np.array(patterns, _bits(dtype)).view(dtype)


def markers(rule, dtype):
    """Values the rule calls missing; the patterns cycle through them."""
    T = np.dtype(dtype).type
    if dtype == np.float64:
        qnan, snan = 0x7FF8000000000000, 0x7FF0000000000001
    else:
        qnan, snan = 0x7FC00000, 0x7F800001
    nans = _from_bits(dtype, qnan, snan, snan | (1 << 20), qnan | 0x1234 | (1 << (63 if dtype == np.float64 else 31)))
    infs = np.array([np.inf, -np.inf], dtype)
    big = np.array([1e36, -1e33, 1e30, np.inf, -np.inf], dtype)
    return {"nan": nans, "inf": infs, "value": np.array([T(1e36)], dtype), "value0": np.array([0.0, -0.0], dtype),
            "abs_ge": big, "nan_inf_abs_ge": np.concatenate([nans, big])}[rule]


def specials(rule, dtype):
    """Values that stay VALID under the rule and must come through bit for bit: -0.0, denormals, and whatever non-finite value
    the rule does not select."""
    tiny = np.finfo(dtype).tiny
    v = [np.array([tiny / 4, -tiny / 1024, np.nextafter(dtype(0), dtype(1))], dtype)]
    if rule != "value0":
        v.append(np.array([-0.0, 0.0], dtype))
    if rule in ("nan", "value", "value0"):
        v.append(np.array([np.inf, -np.inf], dtype))
    if rule in ("inf", "value", "value0", "abs_ge"):
        v.append(markers("nan", dtype))
    if rule in ("nan", "inf", "value0"):
        v.append(np.array([1e36, -1e30], dtype))
    return np.concatenate(v)


def smooth(n, dtype, seed=0):
    """Finite, nonzero data of magnitude below 10 (sf = 1)."""
    i = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = 3.0 + 2.0 * np.sin(i / 97.0) + 1.5 * np.cos(i / 13.0) + 0.01 * rng.standard_normal(n)
    return x.astype(dtype)


def build_input(n, dtype, pat, rule, with_specials=True):
    """(x, miss): smooth data, the rule's markers where the pattern says missing, and -- with_specials -- special values
    that stay valid sprinkled over every eleventh valid element."""
    dtype = np.dtype(dtype).type
    miss = pattern(pat, n)
    x = smooth(n, dtype, seed=n % 1000)
    if with_specials:
        sp = specials(rule, dtype)
        at = np.flatnonzero(~miss)[::11]
        x.view(_bits(dtype))[at] = np.resize(sp.view(_bits(dtype)), at.size)
    mk = markers(rule, dtype)
    at = np.flatnonzero(miss)
    x.view(_bits(dtype))[at] = np.resize(mk.view(_bits(dtype)), at.size)
    return x, miss
