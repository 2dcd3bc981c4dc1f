"""tests/size_cases.py without a GPU: the arithmetic of its workloads, and its predictors against the references computed
directly on miniature big arrays (three repeats of a period of a few tiles, the same construction as F, G2 and G3).

Every predictor must accept the references' outputs on B = expand(S) given the references' outputs on the model S, and must
reject them on the negative control: a B whose last period (and what follows it) is shifted by one block."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mask_cases as M
from tests import ndfix_cases as NF
from tests import ndmask_cases as NM
from tests import ndsummary_cases as NS
from tests import rd_nd_cases as R
from tests import size_cases as Z
from tests.test_gpu_tile_summary import _reduce as flat_reduce

EBS = R.EBS
MINIS = (Z.MINI_F, Z.MINI_G2, Z.MINI_G3)
MODES = ((O.EC, "EC"), (O.QT, "QT"))


def test_workload_arithmetic():
    Z.check_workloads()


def test_expand_and_periodic_agree():
    s = np.arange(7 * 3, dtype=np.float64).reshape(7, 3)
    b = Z.expand(s, 4, 5)
    assert b.shape == (22, 3) and np.array_equal(b[5:10], s[:5]) and np.array_equal(b[20:], s[5:])
    assert Z.periodic(b, s, 4, 5)
    bad = b.copy()
    bad[17, 1] = -0.0 if bad[17, 1] == 0 else -bad[17, 1]
    assert not Z.periodic(bad, s, 4, 5) and not Z.periodic(b[:-1], s, 4, 5)
    nan = s.copy()
    nan[2, 2] = np.nan
    assert Z.periodic(Z.expand(nan, 4, 5), nan, 4, 5)                     # bits, not values
    t = np.array([0, 2, 5, 9, 11], dtype=np.uint32)                       # 3 tiles of the period (9 in all), one of the tail
    c = Z.expand_counted(t, 3, 3, 9)
    assert list(c) == [0, 2, 5, 9, 11, 14, 18, 20, 23, 27, 29]
    assert Z.counted(c.astype(np.uint32), t, 3, 3, 9) and not Z.counted((c + (np.arange(c.size) == 4)).astype(np.uint32), t, 3, 3, 9)
    top = np.array([0, 0xFFFFFFF0], dtype=np.uint32).view(np.int32)       # torch shows the tables as int32
    assert list(Z.expand_counted(top, 1, 0, 0)) == [0, 0xFFFFFFF0]


class Ref:
    """The references' outputs on one array of workload w (flat or tiled), in the shapes the library gives them."""

    def __init__(self, w, x, mode=O.EC):
        self.w, self.x = w, x
        self.c = O.compress_nd(x, Z.EB, mode) if w.tiled else O.compress(x, Z.EB, mode)
        self.out = {"bin_index": self.c.bin_index, "dc": self.c.dc, "ac_exact": self.c.ac_exact}
        self.full = O.decompress_nd(self.c, x.shape) if w.tiled else O.decompress(self.c)
        self.idx = Z.flat_index(self.c.bin_index)

    def records(self):
        return NS.reduce(self.x.shape, self.full, self.x)[0] if self.w.tiled else flat_reduce(self.full, self.x)[0]

    def fix(self, bound):
        if self.w.tiled:
            _, start, off, val = NF.fix_list(self.x, self.full, bound)
            return start, off, val, int(off.size)
        return Z.flat_fix_list(self.x, self.full, bound)


def _masked(w, x):
    """(mask words, count, filled) of the restatements."""
    flags, value, limit = M.RULES[Z.HOLES[0]]
    miss = M.is_missing(x, flags, value, limit)
    if w.tiled:
        return NM.mask_words(miss), int(miss.sum()), NM.fill(x, miss)
    return M.mask_words(miss), int(miss.sum()), M.fill(x, miss)


def _cnt(w, x, eb):
    return (O.compress_nd(x, eb) if w.tiled else O.compress(x, eb)).cnt


@pytest.fixture(scope="module", params=MINIS, ids=lambda w: w.name)
def mini(request):
    w = request.param
    p = Z.pattern(w, "ragged")
    s = Z.model(w, p)
    return w, p, s, Z.expand(s, w.reps, w.period), Z.shifted(w, s)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[1])
def test_streams_decode_and_index(mini, mode):
    w, p, s, b, bad = mini
    rs, rb, rbad = (Ref(w, a, mode[0]) for a in (s, b, bad))
    assert rs.c.sf == rb.c.sf == rbad.c.sf == 10.0
    assert np.array_equal(Z.bits(rs.c.qtable), Z.bits(rb.c.qtable))
    cp, ct = Z.period_counts(rs.c.bin_index, w)
    assert cp > 0 and ct > 0 and cp + ct == rs.c.cnt
    assert rb.c.bin_index.size == w.stream_n and rs.c.bin_index.size == w.model_stream_n
    assert Z.streams_ok(w, rb.out, rb.c.cnt, rs.out, rs.c.cnt)
    assert Z.decode_ok(w, rb.full, rs.full)
    assert Z.index_ok(w, rb.idx, rs.idx, cp) and int(rb.idx[-1]) == rb.c.cnt
    assert np.array_equal(Z.expand_counted(rs.idx, w.reps, w.tiles_per, cp), rb.idx)
    # the control: every predictor says no
    assert not Z.streams_ok(w, rbad.out, rbad.c.cnt, rs.out, rs.c.cnt)
    assert not Z.decode_ok(w, rbad.full, rs.full)
    assert not Z.index_ok(w, rbad.idx, rs.idx, cp)


def test_summary_records_and_correction_list(mini):
    w, p, s, b, bad = mini
    rs, rb, rbad = (Ref(w, a) for a in (s, b, bad))
    assert Z.records_ok(w, rb.records(), rs.records())
    assert not Z.records_ok(w, rbad.records(), rs.records())
    bound = Z.EB * rs.c.sf
    fs, fb, fbad = rs.fix(bound), rb.fix(bound), rbad.fix(bound)
    assert fs[3] > 0 and Z.fix_ok(w, fb, fs)
    assert Z.fix_ok(w, (fb[0], None, None, fb[3]), fs)                     # the count-only form
    assert not Z.fix_ok(w, fbad, fs)


def test_mask_words_filled_copy_and_count():
    for w in MINIS:
        s = Z.model(w, Z.pattern(w, "holes"))
        b, bad = Z.expand(s, w.reps, w.period), Z.shifted(w, s)
        (ms, ks, fs), (mb, kb, fb), (mbad, kbad, fbad) = (_masked(w, a) for a in (s, b, bad))
        assert 0 < ks < s.size and np.isnan(s).any() and (np.abs(s[~np.isnan(s)]) >= 1e30).any()
        assert Z.mask_ok(w, mb, kb, ms, ks) and Z.decode_ok(w, fb, fs)
        assert not Z.mask_ok(w, mbad, kbad, ms, ks) and not Z.decode_ok(w, fbad, fs)


def test_probe_counts(mini):
    w, p, s, b, bad = mini
    cp, cs, cb, cbad = ([_cnt(w, a, eb) for eb in EBS] for a in (p, s, b, bad))
    assert cb == Z.probe_counts(w, cp, cs) and Z.probe_ok(w, cb, cp, cs)
    assert cb[0] > cb[-1]
    assert not Z.probe_ok(w, cbad, cp, cs)
    if w.tiled:                                                            # the sums of squares combine the same way
        for eb in (EBS[0], EBS[9], EBS[-1]):
            sp, ss, sb = (R.predict(a, eb)[1] for a in (p, s, b))
            want = Z.probe_counts(w, [sp], [ss])[0]
            assert abs(sb - want) <= R.SSE_RTOL_F64 * want, (w.name, eb, sb, want)
