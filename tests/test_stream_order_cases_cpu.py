"""The census of what tests/test_gpu_stream_order.py replays with producers pending on the stream (DESIGN.md section 4,
"Stream order"): the subset of the schedules of tests/sequence_cases.py and the one walk added to it.  No GPU."""
import numpy as np

from oracle import oracle as O
from tests import sequence_cases as S


def test_replayed_subset_visits_every_kind_twice_and_every_knob_state():
    d = S.stream_schedules()
    assert list(d)[:5] == list(S.STREAM_REPLAY) == ["walk_9", "walk_10", "d_qt_maxima", "f_same_buffers", "e_after_refusals"]
    a = S.all_schedules()
    assert all(d[n] == a[n] for n in S.STREAM_REPLAY), "the replayed schedules are the call-order ones, unchanged"
    assert len(d) == 6 and d["walk_2_60"] == S.walk(2, 60) and S.HOP_WALK in a
    c = S.census(list(d.values()))
    rare = {k: c["kinds"][k] for k in S.OPS if c["kinds"][k] < 2}
    assert not rare, f"op kinds that occur fewer than twice: {rare}"
    knobs = {(k, v) for k, v in S.STATE_OPS.values() if k}
    assert knobs == set(c["knobs"]) and len(knobs) == 10
    bare = {k: v for k, v in c["knobs"].items() if min(v) < 1}
    assert not bare, f"knob states without a compress and a decode behind them: {bare}"
    assert c["inapplicable"] == 0
    # without the added walk the subset falls short: set_speculation(off) has nothing behind it
    short = S.census([a[n] for n in S.STREAM_REPLAY])
    assert min(short["knobs"][("spec", 0)]) == 0
    print("census:", "min per kind", min(c["kinds"][k] for k in S.OPS), "min per knob state", min(min(v) for v in c["knobs"].values()),
          "ops", sum(len(v) for v in d.values()))


def test_hop_pattern_and_the_subject_two_decades_up():
    hops = [S.hop_stream(i) for i in range(S.WALK_LEN)]
    assert all(h == 2 for h in hops[2::3]) and set(hops) == {0, 1, 2}
    assert all(a != b for a, b in zip(hops, hops[1:])), "every op runs on another stream than the op in front of it"
    two = [h for h in hops if h != 2]
    assert all(a != b for a, b in zip(two, two[1:])), "the two streams alternate"
    big, up = S.SUBJECTS["big"], S.BIG_UP
    assert up.name not in S.SUBJECTS and up.shape == big.shape and up.dtype == big.dtype and up.mode == big.mode == O.EC
    assert np.array_equal(up.x, 100.0 * big.x)
    assert O.compress(up.x, S.EB, O.EC, O.FAST).sf == 100.0 * S.streams("big").sf
