"""The numpy restatement of the missing-value layer (tests/mask_cases.py) pinned against a plain per-block loop on small
arrays: the fill is idempotent, leaves valid elements untouched and leaves no missing element behind; the mask words have the
documented layout; every pattern and rule of the case list builds the input it claims."""
import numpy as np
import pytest

from tests import mask_cases as M

SMALL = (1, 2, 63, 64, 65, 127, 128, 200, 4097)


def _same_bits(a, b):
    U = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and np.array_equal(a.view(U), b.view(U))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rule", sorted(M.RULES))
def test_fill_equals_the_plain_loop(dtype, rule):
    flags, value, limit = M.RULES[rule]
    for n in SMALL:
        for pat in M.PATTERNS:
            x, want = M.build_input(n, dtype, pat, rule)
            miss = M.is_missing(x, flags, value, limit)
            assert np.array_equal(miss, want), (n, pat)           # markers are missing, specials are valid
            f = M.fill(x, miss)
            assert _same_bits(f, M.fill_loop(x, miss)), (n, pat)
            assert _same_bits(f[~miss], x[~miss]), (n, pat)       # valid elements untouched
            again = M.is_missing(f, flags, value, limit)
            nb = -(-n // 64)
            empty = ~np.add.reduceat(~miss, np.arange(0, n, 64)).astype(bool)      # blocks without a valid element get +0.0
            assert empty.shape == (nb,)
            if rule == "value0":
                # ... which this rule calls missing again: the only rule and the only blocks that leave any
                assert np.array_equal(again, np.repeat(empty, 64)[:n] & miss), (n, pat)
                continue
            assert not again.any(), (n, pat)                      # no missing element left
            assert _same_bits(M.fill(f, again), f), (n, pat)      # idempotent
            assert _same_bits(M.fill(f, miss), f), (n, pat)


def test_filled_extremes_are_those_of_the_valid_data():
    x, miss = M.build_input(4097, np.float64, "random30", "value", with_specials=False)
    f = M.fill(x, miss)
    assert miss.any() and not miss.all()
    assert np.abs(f).max() == np.abs(x[~miss]).max() and np.abs(f).min() == np.abs(x[~miss]).min()
    # a block without any valid element takes +0.0: the maximum is still the valid data's, the minimum is then 0
    x, miss = M.build_input(4097, np.float64, "blobs", "value", with_specials=False)
    f = M.fill(x, miss)
    assert miss.reshape(-1)[:4096].reshape(64, 64).all(axis=1).any()
    assert np.abs(f).max() == np.abs(x[~miss]).max() and np.abs(f).min() == 0.0


def test_mask_word_layout():
    n = 130
    miss = np.zeros(n, bool)
    miss[[0, 5, 63, 64, 129]] = True
    w = M.mask_words(miss)
    assert w.dtype == np.uint64 and w.tolist() == [(1 << 0) | (1 << 5) | (1 << 63), 1 << 0, 1 << 1]
    assert np.array_equal(M.mask_bits(w, n), miss)
    for n in SMALL:
        for pat in M.PATTERNS:
            miss = M.pattern(pat, n)
            w = M.mask_words(miss)
            assert w.size == -(-n // 64) and np.array_equal(M.mask_bits(w, n), miss)
            if n % 64:
                assert int(w[-1]) >> (n % 64) == 0                # bits beyond n are 0


def test_patterns_cover_what_they_name():
    n = 64 * 777 + 45
    assert not M.pattern("none", n).any() and M.pattern("all", n).all()
    assert M.pattern("first", n).nonzero()[0].tolist() == [0] and M.pattern("last", n).nonzero()[0].tolist() == [n - 1]
    wb = M.pattern("whole_block", n)
    assert wb[64:128].all() and wb.sum() == 64
    lg = M.pattern("leading_gap", n).reshape(-1)[:64 * 777].reshape(777, 64)
    assert lg[:, 0].all() and not lg[:, 63].any()
    tg = M.pattern("trailing_gap", n)[:64 * 777].reshape(777, 64)
    assert tg[:, 63].all() and not tg[:, 0].any()
    ab = M.pattern("across_boundaries", n)
    assert ab[63] and ab[64] and ab[4095] and ab[4096] and ab[4026] and not ab[4025]
    la = M.pattern("last_block_all", n)
    assert la[64 * 777:].all() and not la[:64 * 777].any()
    ll = M.pattern("last_block_leading", n)
    assert ll[64 * 777] and not ll[n - 1]
    r = M.pattern("random30", n).mean()
    assert 0.28 < r < 0.32
    b = M.pattern("blobs", n)
    assert 0.1 < b.mean() < 0.5 and np.count_nonzero(np.diff(b.astype(np.int8))) < n // 20      # runs, not salt and pepper
