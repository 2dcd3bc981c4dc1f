"""Any order of calls on one context gives a fresh context's bits ("Call order").

One test per schedule of tests/sequence_cases.py: eight random walks over the whole vocabulary of dctz_amd.Context, and the
directed schedules (capacity ladders, element-type flips, changing short blocks, alternating QT maxima, every family after
every refusal and after a launch that gave up, decodes after the buffers of their streams were written again, two contexts
on two streams).  Each test has one context for the whole schedule.  After every op its results are compared bit for bit
with what sequence_cases expects (E1: the oracle and the numpy models; E2: the same op as the first work call of a fresh
context), and every output lies in an arena of 0xA5 bytes whose guard bands -- 256 bytes on both sides of every output --
and whose unused space are checked, with the tail of AC_exact beyond cnt: a size or a capacity left over from an earlier
call that stays inside the allocation shows there.  Further tests pin the paths the subjects are meant for, and the wrap
of the one-launch tag.

A failure names the schedule, the index of the op, the five ops in front of it and the first differing element; it is
replayed with  S.all_schedules()[name][:index + 1].

(The streams the deflate ops write are allocated by the wrapper with torch itself and lie outside the arena.)"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sequence_cases as S
from tests.sequence_runner import (Arena, _ArenaTorch, Mismatch, Runner, _IMPL, _e2,       # noqa: F401  (the runner: tests/sequence_runner.py)
                                   GUARD, FILL, ONE_CALLS, ONE_GAVE_UP, SPEC_HITS, MEMO, HIST_HITS, VARIANT, E2)

pytestmark = pytest.mark.gpu


def _inputs_intact(r, where):
    for (name, raw), t in r.inputs.items():
        s = S.SUBJECTS[name]
        assert np.array_equal(t.cpu().numpy().view(np.uint8), (s.raw if raw else s.x).view(np.uint8)), f"{where}: the input {name} was modified"


def _play(name, sched):
    contexts = 1 + max(a.get("ctx", 0) for _, _, a in sched)
    import torch
    rs = [Runner(e2=_e2, stream=torch.cuda.Stream() if contexts > 1 else None) for _ in range(contexts)]
    ran = 0
    try:
        if contexts == 1:
            for i, op in enumerate(sched):
                rs[0].run(op, f"schedule {name}, op {i}")
                ran += 1
        else:                                             # the ops of a round are all launched before any result is looked at
            for i in range(0, len(sched), contexts):
                rnd = sched[i:i + contexts]
                for op in rnd:
                    rs[op[2]["ctx"]].launch(op, f"schedule {name}, round at op {i}")
                for j, op in enumerate(rnd):
                    rs[op[2]["ctx"]].finish(f"schedule {name}, op {i + j} (context {op[2]['ctx']})")
                    ran += 1
        for r in rs:
            _inputs_intact(r, f"schedule {name}")
    finally:
        for r in rs:
            r.close()
    assert ran == len(sched), "the runner leaves no op out"


SCHEDULES = S.all_schedules()


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule(name):
    _play(name, SCHEDULES[name])


def test_two_fresh_contexts_agree_on_every_e2_op():
    """What E2 rests on: the ops compared with a fresh context's result are repeatable between fresh contexts."""
    rng = np.random.default_rng(1)
    for kind, (_, _, applies, source) in S.OPS.items():
        if source != "E2" and kind != "compress_coef":
            continue
        name = next(n for n in ("b12325", "t3a") if S.applies(kind, n))
        op = (kind, name, S.make_args(kind, name, rng))
        first = dict(_e2(op))
        again = {}
        r = Runner(record=again, persistent=4 << 20, transient=16 << 20)
        try:
            r.run(op, "second fresh context")
        finally:
            r.close()
        assert first.keys() == again.keys() and len(first) > 0
        for k in first:
            assert np.array_equal(first[k].reshape(-1).view(np.uint8), again[k].reshape(-1).view(np.uint8)), (kind, k)


# ---- the paths the subjects are meant for ---------------------------------------------------------------------------------------
@pytest.fixture()
def runner():
    r = Runner(e2=_e2)
    yield r
    r.close()


def test_path_one_launch(runner):
    """Every flat subject takes the one-launch kernels on a context as it is created (counter 0, the kernel's name)."""
    ctx = runner.ctx
    for name in S.FLAT:
        calls = ctx.counter(ONE_CALLS)
        runner.run(S.op("compress", name), "one launch")
        assert ctx.counter(ONE_CALLS) == calls + 1 and ctx.last_kernel(0).startswith("k_compress_one<"), (name, ctx.last_kernel(0))
        runner.run(S.op("decompress", name), "one launch")
        assert ctx.counter(ONE_CALLS) == calls + 2 and ctx.last_kernel(1).startswith("k_decompress_one<"), (name, ctx.last_kernel(1))
    assert ctx.counter(ONE_GAVE_UP) == 0
    calls = ctx.counter(ONE_CALLS)
    members = [S.ONE_WIDEST, "big32", "a2597d"]
    runner.run(S.op("compress_batch", members[0], members=members), "one launch")
    assert ctx.counter(ONE_CALLS) > calls and ctx.last_kernel(2).startswith("k_compress_one_batch<double") and ctx.last_kernel(3).startswith("k_compress_one_batch<float")


def test_path_chain_and_memo(runner):
    """With one launch off every flat subject takes the chain; the memo subjects decode on the last compress call's counts."""
    ctx = runner.ctx
    runner.run(S.op("one_off"), "chain")
    for name in S.FLAT:
        calls, memo = ctx.counter(ONE_CALLS), ctx.counter(MEMO)
        runner.run(S.op("compress", name), "chain")
        s = S.SUBJECTS[name]
        assert ctx.counter(ONE_CALLS) == calls and not ctx.last_kernel(0).startswith("k_compress_one"), (name, ctx.last_kernel(0))
        assert s.n < 64 or ctx.last_kernel(0).startswith("k_compress<"), (name, ctx.last_kernel(0))      # (a short block alone: no big kernel)
        runner.run(S.op("decompress", name), "chain")
        assert ctx.counter(ONE_CALLS) == calls and not ctx.last_kernel(1).startswith("k_decompress_one"), (name, ctx.last_kernel(1))
        assert s.n < 64 or ctx.last_kernel(1).startswith("k_decompress"), (name, ctx.last_kernel(1))
        hit = s.dtype == S.F64 and s.mode == O.EC and s.n % 64 == 0
        assert ctx.counter(MEMO) == memo + (1 if hit else 0), name
        assert ("true" in ctx.last_kernel(1)) == hit, (name, ctx.last_kernel(1))
    assert {n for n in S.FLAT if S.SUBJECTS[n].dtype == S.F64 and S.SUBJECTS[n].mode == O.EC and S.SUBJECTS[n].n % 64 == 0} == set(S.MEMO_PAIR)
    runner.run(S.op("split_on"), "chain")
    runner.run(S.op("compress", "c12288"), "chain")
    assert ctx.last_kernel(0).startswith("k_compress_eo<") and ctx.counter(3) == 1


def test_path_sampled_and_remembered_sf(runner):
    """On the chain with set_speculation(True, 1 << 18) the two large subjects take a sampled guess of sf (counter 6), and from
    the third call on the same input the remembered one (counter 18)."""
    ctx = runner.ctx
    runner.run(S.op("one_off"), "sf")
    runner.run(S.op("spec_on"), "sf")
    for name in ("big", "big32"):
        for i in range(4):
            hits, hist = ctx.counter(SPEC_HITS), ctx.counter(HIST_HITS)
            runner.run(S.op("compress", name), "sf")
            assert ctx.counter(SPEC_HITS) == hits + 1, (name, i)
            assert ctx.counter(HIST_HITS) == hist + (1 if i >= 2 else 0), (name, i)
        assert ctx.counter(7) == 0 and ctx.counter(19) == 0
    hits = ctx.counter(SPEC_HITS)
    runner.run(S.op("compress", "c12288"), "sf")             # below the threshold: the plain statistics pass
    assert ctx.counter(SPEC_HITS) == hits


def test_one_launch_tag_wraps_onto_a_cleared_board(runner):
    """S.epoch_wrap(): a launch that takes tag 1 again finds no granule of the launches that carried tag 1 before it."""
    ctx = runner.ctx
    for i, op in enumerate(S.epoch_wrap()):
        calls = ctx.counter(ONE_CALLS)
        runner.run(op, f"epoch wrap, op {i}")
        if op[0] != "epoch":
            assert ctx.counter(ONE_CALLS) > calls, (i, op)
    assert ctx.counter(ONE_GAVE_UP) == 0
