"""The census of tests/sequence_cases.py: what the random walks of tests/test_gpu_call_sequences.py visit, that the subjects
have the properties the schedules rely on, and that every schedule is the same data every time.  No GPU."""
import numpy as np

from oracle import oracle as O
from tests import sequence_cases as S


def _walks():
    return [S.walk(seed) for seed in S.WALK_SEEDS]


def test_walks_visit_every_kind_pair_subject_and_knob_state():
    assert len(S.FAMILIES) == 12 and len(S.WALK_SEEDS) == 8 and all(len(w) == S.WALK_LEN == 120 for w in _walks())
    c = S.census(_walks())
    rare = {k: v for k, v in c["kinds"].items() if v < 5}
    assert not rare, f"op kinds that occur fewer than 5 times: {rare}"
    missing = [p for p, v in c["pairs"].items() if v == 0]
    assert len(c["pairs"]) == 144 and not missing, f"ordered pairs of families never taken: {missing}"
    assert c["compressed"] == set(S.SUBJECTS), set(S.SUBJECTS) - c["compressed"]
    assert c["decoded"] == set(S.SUBJECTS), set(S.SUBJECTS) - c["decoded"]
    bare = {k: v for k, v in c["knobs"].items() if min(v) < 1}
    assert len(c["knobs"]) == 10 and not bare, f"knob states without a compress and a decode behind them: {bare}"
    print("census:", "min per kind", min(c["kinds"].values()), "min per pair", min(c["pairs"].values()),
          "min per knob state", min(min(v) for v in c["knobs"].values()))


def test_nothing_emitted_that_does_not_apply():
    for name, sched in S.all_schedules().items():
        assert S.census([sched])["inapplicable"] == 0, name
        for kind, subject, args in sched:
            assert kind in S.KINDS and (subject is None or subject in S.SUBJECTS), (name, kind, subject)
            if kind in ("compress_batch", "decompress_batch"):
                m = [S.SUBJECTS[n] for n in args["members"]]
                assert 1 <= len(m) <= 3 and len({s.mode for s in m}) == 1 and all(s.flat for s in m), (name, args)
                assert len(set(args.get("slots", args["members"]))) == len(m)
                if name.startswith("walk"):           # 3 items of mixed dtype
                    assert len(m) == 3 and len({s.dtype for s in m}) == 2, (name, args)
            if "slot" in args:                        # buffers that two subjects share hold either of them
                assert subject in S.MEMO_PAIR and args["slot"] == "shared"
    for kind, subject, args in S.epoch_wrap():
        assert kind == "epoch" or S.applies(kind, subject)


def test_schedules_are_reproducible_from_their_seeds():
    assert S.all_schedules() == S.all_schedules()
    for seed in S.WALK_SEEDS:
        assert S.walk(seed) == S.walk(seed) and S.walk(seed) != S.walk(seed + 1000)
    assert S.epoch_wrap() == S.epoch_wrap()
    import json
    json.dumps(S.all_schedules())                     # plain data


def test_directed_schedules_are_what_they_claim():
    d = S.directed()
    assert sorted(k[0] for k in d) == list("aabcdefg")
    # (a) first and last subject of every kind's run: large, ..., large / small, ..., small
    for name, first in (("a_ladder_large_first", "big"), ("a_ladder_small_first", "a27")):
        runs = [s for k, s, _ in d[name] if k == "compress"]
        assert runs[0] == first and S.SUBJECTS[runs[0]].n != S.SUBJECTS[runs[1]].n
    # (b) / (d): the pairs alternate, on one launch and on the chain
    for name, pair, times in (("b_dtype_flip_qt", S.DTYPE_PAIR, 3), ("d_qt_maxima", S.QT_PAIR, 6)):
        seq = [s for k, s, _ in d[name] if k == "compress" and s in pair]
        assert seq[:2 * times] == list(pair) * times and seq[2 * times:4 * times] == list(pair) * times
        assert [k for k, _, _ in d[name] if k in ("one_on", "one_off")][:2] == ["one_on", "one_off"]
    # (e) every refusal, and the withheld granule, is followed by one op of every family
    e = d["e_after_refusals"]
    for i, (kind, _, _) in enumerate(e):
        if kind in S.REFUSALS or kind == "withheld":
            assert {S.family(k) for k, _, _ in e[i + 1:i + 13]} == set(S.FAMILIES), (i, kind)
    assert {k for k, _, _ in e} >= set(S.REFUSALS) | {"withheld"}
    # (f) B goes into the buffers A's streams were decoded from
    f = d["f_same_buffers"]
    a, b = S.MEMO_PAIR
    assert (("compress", b, {"slot": "shared"}) in f) and (("compress", a, {"slot": "shared"}) in f) and (("compress", b, {}) in f)
    # (g) the contexts alternate
    assert [g[2]["ctx"] for g in d["g_two_contexts"]] == [0, 1] * 40


def test_subjects_have_the_properties_the_schedules_rely_on():
    sub = S.SUBJECTS
    # every (dtype, mode) at least twice among the flat subjects, with different short blocks
    for dt in (S.F32, S.F64):
        for mode in (O.EC, O.QT):
            rems = {sub[n].n % 64 for n in S.FLAT if sub[n].dtype == dt and sub[n].mode == mode}
            assert len(rems) >= 2, (dt, mode, rems)
    a, b = S.QT_PAIR
    assert sub[a].n == sub[b].n and sub[a].dtype == sub[b].dtype and sub[a].mode == sub[b].mode == O.QT
    qa, qb = S.streams(a).qtable_raw, S.streams(b).qtable_raw
    both = (qa > 0) & (qb > 0)
    assert both.sum() >= 32 and (qa[both] > 4 * qb[both]).all(), (qa / np.where(qb > 0, qb, 1)).min()
    assert not np.array_equal(S.streams(a).qtable, S.streams(b).qtable)
    a, b = S.DTYPE_PAIR
    assert sub[a].n == sub[b].n and sub[a].dtype != sub[b].dtype and sub[a].mode == sub[b].mode
    a, b = S.REM_PAIR
    assert sub[a].dtype == sub[b].dtype and 0 != sub[a].n % 64 != sub[b].n % 64 != 0
    a, b = S.MEMO_PAIR
    assert sub[a].shape == sub[b].shape and sub[a].dtype == sub[b].dtype == S.F64 and sub[a].mode == sub[b].mode == O.EC and sub[a].n % S.TILE == 0
    assert not np.array_equal(S.streams(a).bin_index, S.streams(b).bin_index) and S.streams(a).cnt != S.streams(b).cnt
    # every stream tile stores some coefficients exactly, and not every tile the same number
    for name in sub:
        cnt = S.tile_counts(S.streams(name).bin_index)
        assert int(cnt.sum()) == S.streams(name).cnt == S.index(name)[-1] and (cnt[:-1] > 0).all(), (name, cnt)
        assert cnt[-1] > 0 or sub[name].n % S.TILE == 1, (name, cnt)       # (a last tile of one element has no position j != 0)
        if cnt.size > 1:
            assert np.unique(cnt).size > 1, (name, cnt)
    # holes, and arrays without any
    for name, s in sub.items():
        w, count, filled = S.mask(name)
        assert (count > 0) == s.holes and count == int((np.abs(s.raw) >= S.LIMIT).sum())
        assert np.abs(filled).max() < 100.0
    assert sum(s.holes for s in sub.values()) == 2 and {sub[n].flat for n in sub if sub[n].holes} == {True, False}
    # the sampled guess of sf: n >= 4 * chunk * spec_group in either element type (a chunk is 4 KiB, a group 64 chunks)
    for name in ("big", "big32"):
        assert sub[name].n >= S.SPEC_MIN and sub[name].n >= 4 * (4096 // sub[name].dtype.itemsize) * 64 and sub[name].n <= 1 << 19
    assert all(s.n <= 1 << 19 for s in sub.values())
    # the correction lists are neither empty nor everything
    for name in sub:
        for mult in (0.25, 0.5):
            start, off, val = S.fix_list(name, mult)
            assert 0 < off.size < sub[name].n and start[-1] == off.size == val.size
