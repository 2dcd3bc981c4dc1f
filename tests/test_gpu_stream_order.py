"""Stream order ("Stream order"): every entry point with its producers still pending on the stream when
the library is entered, and with its buffers recycled the moment it returns.

include/dctz_hip.h promises that a call reads its inputs behind whatever is queued on the context's stream and that its
outputs are complete in stream order, not at return.  The other GPU tests enter the library on an idle stream (inputs come
from synchronous uploads) and read results back through .cpu(), which drains it: a kernel on a side stream that runs ahead
of a producer, or work left on a stream that is never joined back, reads and writes the right bytes there.  Here

  before a call   every device buffer the call reads holds a DECOY and the stream is drained; then, directly in front of the
                  C call (Context._bind_stream is the first statement of every wrapper method and is hooked on the runner's
                  context), a delay, the device-to-device copies that put the true bytes back from shadow copies and an
                  event are queued on the context's stream without a host wait; event.query() is recorded and must be False;
  after a call    as soon as the wrapper returns, clones of every tensor in the op's checks are queued on the same stream,
                  then every persistent input and every slot the op did not write is overwritten with its decoy again;
                  finish() compares the clones.

A decoy is harmless when read early: zero bytes for indices, list tables and offsets, the arena's 0xA5 for values and bin
ids (bin id 165 and -2.9e-16 are valid data) -- an early reader gets wrong values or a checked refusal, never an offset out
of range.  (The overwrite behind a call uses the same decoys, zeros for the index tables too, for the same reason.)  The
delay is a fixed number of device-to-device copies, sized once per module with device events.

The negative controls repeat the pre-step with the producer on ANOTHER stream than the context's: nothing orders the two,
the library legitimately runs ahead, and the op must end in a Mismatch.  A control that passes means the delay shows nothing.
"""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

from dctz_amd import hip as H
from oracle import oracle as O
from tests import sequence_cases as S
from tests.sequence_runner import FILL, HIST_HITS, MEMO, ONE_CALLS, SPEC_HITS, Arena, Mismatch, Runner, _ArenaTorch, _e2

pytestmark = pytest.mark.gpu

REDO, HIST_MISSES = 17, 19              # dctzhip_debug_counter
DELAY_MS = 5.0                          # what the delay is sized for; a warm call queues its kernels within tens of microseconds
TALLY = {"work ops": 0, "pending at entry": 0}


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _decoy(t):
    """0xA5 for values and bin ids, zero bytes for indices, list tables and offsets."""
    import torch
    flat = t.reshape(-1)
    if t.dtype.is_floating_point or t.dtype == torch.uint8:
        flat.view(torch.uint8).fill_(FILL)
    else:
        flat.zero_()


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.size == want.size and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(_bits(got), _bits(want))


class Delay:
    """A bounded amount of ordinary work on the current stream: `copies` device-to-device copies of 512 MiB -- far beyond the
    last-level cache, so that a copy takes the device many times what it takes the host to queue it."""
    NBYTES = 512 << 20

    def __init__(self, device):
        import time
        import torch
        self.a = torch.empty(self.NBYTES, dtype=torch.uint8, device=device)
        self.b = torch.zeros(self.NBYTES, dtype=torch.uint8, device=device)
        self.copies = 4
        self._timed()                                    # (warm)
        per = self._timed() / self.copies
        self.copies = max(2, int(math.ceil(DELAY_MS / per)))
        self.ms = self._timed()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.queue()
        self.host_ms = (time.perf_counter() - t0) * 1e3  # what the host needs to queue it
        torch.cuda.synchronize()

    def _timed(self):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.queue()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def queue(self):
        for _ in range(self.copies):
            self.a.copy_(self.b)


@pytest.fixture(scope="module")
def delay():
    import torch
    d = Delay(torch.device("cuda", 0))
    print(f"stream-order delay: {d.copies} device-to-device copies of {d.NBYTES >> 20} MiB, {d.ms:.2f} ms measured on the device, queued in {d.host_ms:.3f} ms")
    assert d.ms >= 0.8 * DELAY_MS and d.host_ms <= 0.25 * d.ms, "the delay is over before the library can be entered behind it"
    yield d
    print(f"stream-order tally: {TALLY['pending at entry']} of {TALLY['work ops']} work ops entered the library with their producers pending")
    assert TALLY["pending at entry"] == TALLY["work ops"] > 0


class Gate:
    """The hook on one context's _bind_stream.  Once armed, the next call of it -- the first statement of a wrapper method,
    directly in front of the C call -- queues the delay, the copies of `pairs()` (destination, source) and an event on the
    context's stream (or on `producer`, the negative control), records event.query() and disarms."""

    def __init__(self, ctx, delay):
        import torch
        self.torch, self.delay = torch, delay
        self.armed, self.fired, self.pending = None, 0, []
        bind = ctx._bind_stream

        def hooked():
            bind()
            if self.armed is not None:
                armed, self.armed = self.armed, None
                self._queue(*armed)
        ctx._bind_stream = hooked

    def arm(self, pairs, producer=None, drain=True):
        self.armed = (pairs, producer, drain)
        self.fired = 0

    def disarm(self):
        self.armed = None
        return self.fired

    def _queue(self, pairs, producer, drain):
        t = self.torch
        if drain:
            t.cuda.current_stream().synchronize()        # the decoys are in place
        with (t.cuda.stream(producer) if producer is not None else contextlib.nullcontext()):
            self.delay.queue()
            for dst, src in pairs():
                dst.copy_(src)
            ev = t.cuda.Event()
            ev.record()
        self.pending.append(not ev.query())
        self.fired += 1


class StreamRunner(Runner):
    """Runner with every op wrapped as the module's docstring says.  drain=False (the stream hops): no host wait in front of
    a call -- the decoys are the ones the last call's post-step left -- and the context is bound first, so that what the
    caller itself does to the buffers is ordered behind the call before."""

    def __init__(self, delay, producer=None, drain=True, **kw):
        super().__init__(**kw)
        self.gate = Gate(self.ctx, delay)
        self.producer, self.drain = producer, drain
        self.shadow = {}                                  # key -> (the live buffer, its true bytes)
        self.transients, self.written = [], set()
        self.work = 0
        self.arenas = [self.tmp]
        self._track(self.tmp)

    def _track(self, arena):
        put = arena.put

        def tracked(a, *args, **kw):
            d = put(a, *args, **kw)
            if self.gate.armed is not None:               # (behind the call's queue nothing would put the true bytes back)
                self.transients.append((d, d.clone()))
                _decoy(d)
            return d
        arena.put = tracked

    def second_arena(self, nbytes=20 << 20):
        with self._on_stream():
            self.arenas.append(Arena(self.ctx.device, nbytes))
        self._track(self.arenas[-1])

    def use_arena(self, i):
        self.tmp = self.arenas[i]
        self.ctx.torch = _ArenaTorch(self.tmp)

    def _adopt(self, key, t):
        self.shadow[key] = (t, t.clone())
        if self.gate.armed is not None:                   # (as above; the post-step leaves the decoy then)
            _decoy(t)

    def x(self, name, raw=False):
        new = (name, raw) not in self.inputs
        t = super().x(name, raw)
        if new:
            self._adopt(("input", name, raw), t)
        return t

    def index(self, name):
        new = name not in self.indices
        t = super().index(name)
        if new:
            self._adopt(("index", name), t)
        return t

    def slot(self, slot, name, for_decode=False):
        new = slot not in self.slots
        b = super().slot(slot, name, for_decode)
        if new:
            for k, v in b.items():
                self._adopt(("slot", slot, k), v)
        return b

    def poison(self, b):
        self.written.update(k for k, v in self.slots.items() if v is b)
        super().poison(b)

    def _is_written(self, key):
        return key[0] == "slot" and key[1] in self.written

    def _pairs(self):
        return [p for key, p in self.shadow.items() if not self._is_written(key)] + self.transients

    def launch(self, op, where=""):
        self.written, self.transients[:] = set(), []
        with self._on_stream():
            if self.drain:
                for live, _ in self.shadow.values():
                    _decoy(live)
                self.torch.cuda.current_stream().synchronize()
            else:
                self.ctx._bind_stream()
            self.gate.arm(self._pairs, self.producer, self.drain)
            try:
                super().launch(op, where)
            finally:
                fired = self.gate.disarm()
            op_, checks = self.pending
            checks = [(label, got.clone() if hasattr(got, "is_cuda") else got, want) for label, got, want in checks]
            for key, (live, true) in self.shadow.items():
                if self._is_written(key):
                    true.copy_(live)
                else:
                    _decoy(live)
            self.pending = (op_, checks)
        if op[0] in S.OPS or op[0] == "withheld":
            assert fired == 1, f"{where}: {op[0]} never reached a wrapper method"
            self.work += 1

    def settle(self, where):
        """The end of a schedule: every work op found its producers pending; the shadows are still the subjects' bytes."""
        self.torch.cuda.synchronize()
        pending = self.gate.pending
        TALLY["work ops"] += len(pending)
        TALLY["pending at entry"] += sum(pending)
        assert len(pending) >= self.work and all(pending), f"{where}: {len(pending) - sum(pending)} of {len(pending)} calls were entered behind a finished producer"
        for key, (_, true) in self.shadow.items():
            if key[0] == "input":
                s = S.SUBJECTS[key[1]]
                assert _same(true.cpu().numpy(), s.raw if key[2] else s.x), f"{where}: the shadow of {key[1]} was modified"
            elif key[0] == "index":
                assert _same(true.cpu().numpy(), S.index(key[1])), f"{where}: the shadow of the index of {key[1]} was modified"


# ---- the existing vocabulary, replayed ----------------------------------------------------------------------------------------
SCHEDULES = S.stream_schedules()


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule_with_producers_pending(delay, name):
    sched = SCHEDULES[name]
    r = StreamRunner(delay, e2=_e2)
    ran = 0
    try:
        for i, op in enumerate(sched):
            r.run(op, f"schedule {name}, op {i}")
            ran += 1
        r.settle(f"schedule {name}")
        work = sum(1 for k, _, _ in sched if k in S.OPS or k == "withheld")
        assert r.work == work
        print(f"schedule {name}: {sum(r.gate.pending)} of {len(r.gate.pending)} calls ({work} work ops) entered with the producer pending")
    finally:
        r.close()
    assert ran == len(sched), "the runner leaves no op out"


CONTROLS = [S.op("compress", "a2597"), S.op("decompress", "c12288"), S.op("box_nd", "t3r", lo=[1, 2, 3], hi=[8, 13, 22]),
            S.op("fixup_apply", "a2597", mult=0.5), S.op("mask_apply", "h2597", fill=-1.0),
            S.op("compress_batch", "a2597", members=["a2597", "a2597d", "a91"])]


@pytest.mark.parametrize("op", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_negative_control_a_producer_on_another_stream_is_overtaken(delay, op):
    """The same pre-step with the producer on S1 and the context on S2: the call runs ahead and must not give the true result.
    The op runs once behind a producer on its own stream first -- it is right there, and the context's one-time allocations
    and uploads are made -- so the two runs differ in the producer's stream alone."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r = StreamRunner(delay, stream=s2, e2=_e2)
    try:
        r.run(op, f"positive control {op[0]}")
        r.settle(f"positive control {op[0]}")
        r.producer = s1
        with pytest.raises(Mismatch):
            r.run(op, f"negative control {op[0]}")
        torch.cuda.synchronize()
        assert r.gate.pending == [True, True]
    finally:
        torch.cuda.synchronize()
        r.close()


# ---- moving a context between streams -----------------------------------------------------------------------------------------
def test_bind_orders_the_new_stream_behind_the_old(delay):
    """Context._bind_stream under another current stream: the new stream waits for what the context left on the old one."""
    import torch
    import dctz_amd
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ctx = dctz_amd.Context(0)
    with torch.cuda.stream(s2):                           # (a stream's first use may take the runtime longer than the delay)
        torch.zeros(64, device=ctx.device)
    try:
        name = "a2597d"
        s, c = S.SUBJECTS[name], S.streams(name)
        with torch.cuda.stream(s1):
            ctx._bind_stream()
            xd = torch.from_numpy(s.x.copy()).to(ctx.device)
            torch.cuda.synchronize()
            delay.queue()
            ev = torch.cuda.Event()
            ev.record()
        with torch.cuda.stream(s2):
            ctx._bind_stream()
        busy, pending = not s2.query(), not ev.query()
        assert pending, "the delay on S1 was over before S2 could be asked"
        assert busy, "S2 is idle while S1 is busy: nothing orders the context's new stream behind its old one"
        assert ctx._bound == s2.cuda_stream and ctx._stream == s2
        s1.synchronize()
        s2.synchronize()
        with torch.cuda.stream(s2):
            out, info = ctx.compress(xd, S.EB, s.mode)
            rec = ctx.decompress(out, info.cnt, s.n, _tdt(s.dtype), S.EB, info.sf, s.mode)
            assert (info.sf, info.cnt) == (c.sf, c.cnt)
            assert _same(out["bin_index"].cpu().numpy(), c.bin_index) and _same(out["dc"].cpu().numpy(), c.dc)
            assert _same(out["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact) and _same(rec.cpu().numpy(), S.decode(name))
    finally:
        torch.cuda.synchronize()
        ctx.close()


def test_h_stream_hops(delay):
    """walk_11 with the ops alternating between two streams and every third op on the legacy default stream; an op is
    launched before the results of the op in front of it are looked at, and nothing but finish() waits on the host."""
    import torch
    sched = S.all_schedules()[S.HOP_WALK]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
    assert streams[2].cuda_stream == 0
    r = StreamRunner(delay, drain=False, e2=_e2, stream=streams[0])
    r.second_arena()
    ran, prev, used = 0, None, [None, None]
    try:
        for i, op in enumerate(sched):
            r.stream = streams[S.hop_stream(i)]
            r.use_arena(i % 2)
            if used[i % 2] is not None:                   # (the caller's own hand-over of its arena; that stream was drained by finish)
                r.stream.wait_stream(used[i % 2])
            used[i % 2] = r.stream
            r.launch(op, f"h_stream_hops, op {i}")
            cur = (r.pending, r.stream, r.tmp)
            if prev is not None:
                r.pending, r.stream, r.tmp = prev
                r.finish(f"h_stream_hops, op {i - 1}")
                ran += 1
            r.pending, r.stream, r.tmp = None, cur[1], cur[2]
            prev = cur
        r.pending, r.stream, r.tmp = prev
        r.finish(f"h_stream_hops, op {len(sched) - 1}")
        ran += 1
        r.settle("h_stream_hops")
        hops = sum(1 for i in range(1, len(sched)) if S.hop_stream(i) != S.hop_stream(i - 1))
        assert hops == len(sched) - 1 and {S.hop_stream(i) for i in range(len(sched))} == {0, 1, 2}
    finally:
        torch.cuda.synchronize()
        r.close()
    assert ran == len(sched), "the runner leaves no op out"


# ---- time steps: one input buffer and one set of stream buffers, contents rotated behind the delay --------------------------
class Steps:
    """A context, one input buffer, one set of stream buffers and one output; compress / decompress with their producers
    pending, the results cloned on the stream the moment the calls return."""

    def __init__(self, delay, n, dtype):
        import torch
        import dctz_amd
        self.torch = torch
        self.ctx = dctz_amd.Context(0)
        self.gate = Gate(self.ctx, delay)
        dev, self.tdt = self.ctx.device, _tdt(dtype)
        self.n = n
        self.xin = torch.full((n,), 0, dtype=self.tdt, device=dev)
        self.dst = torch.empty(n, dtype=self.tdt, device=dev)
        self.b = self.ctx.alloc_outputs(n)
        for t in (self.xin, self.dst) + tuple(self.b.values()):
            t.view(torch.uint8).fill_(FILL)
        self.true = {}

    def dev(self, key, a):
        if key not in self.true:
            self.true[key] = self.torch.from_numpy(np.array(a, copy=True)).to(self.ctx.device)
        return self.true[key]

    def compress(self, key, x, mode):
        """The input buffer still holds the last step's content; this step's arrives behind the delay."""
        src = self.dev(key, x)                            # (an upload the first time: ahead of the delay)
        self.gate.arm(lambda: [(self.xin, src)], drain=False)
        _, info = self.ctx.compress(self.xin, S.EB, mode, out=self.b)
        assert self.gate.disarm() == 1
        return info, {k: v.clone() for k, v in self.b.items()}

    def decompress(self, info, mode, rewrite=(), cnt=None):
        """Behind the compress call's tail and a delay; rewrite: (stream, true bytes) put into the stream buffers behind it."""
        pairs = [(self.b[k][:a.numel()], a) for k, a in rewrite]
        self.gate.arm(lambda: pairs, drain=False)
        q = np.array(info.qtable[:]) if mode == O.QT else None
        self.ctx.decompress(self.b, info.cnt if cnt is None else cnt, self.n, self.tdt, S.EB, info.sf, mode, qtable=q, dst=self.dst)
        assert self.gate.disarm() == 1
        rec = self.dst.clone()
        self.dst.view(self.torch.uint8).fill_(FILL)
        return rec

    def close(self):
        self.torch.cuda.synchronize()
        pending = self.gate.pending
        TALLY["work ops"] += len(pending)
        TALLY["pending at entry"] += sum(pending)
        self.ctx.close()
        assert all(pending)


def _check_streams(where, info, got, c):
    assert (info.sf, int(info.cnt)) == (c.sf, int(c.cnt)), (where, info.sf, info.cnt, c.sf, c.cnt)
    assert _same(got["bin_index"].cpu().numpy(), c.bin_index), where
    assert _same(got["dc"].cpu().numpy(), c.dc), where
    assert _same(got["ac_exact"][:c.cnt].cpu().numpy(), c.ac_exact), where
    if c.mode == O.QT:
        assert _same(np.array(info.qtable[:], dtype=c.qtable.dtype), c.qtable), where


def _flag_moved(c):
    """tests/test_gpu_decode_memo.py: the streams with one flag moved from tile 0 to the last tile -- the same total, other
    counts per tile -- and what the oracle decodes from them."""
    j = np.arange(c.bin_index.size) % 64
    pos = lambda b: np.flatnonzero((b == 255) & (j != 0))                  # noqa: E731
    bin2 = c.bin_index.copy()
    flags = pos(bin2)
    e1 = int(flags[0])
    assert e1 < S.TILE
    bin2[e1] = 0
    ac2 = np.delete(c.ac_exact, 0)
    last = (c.bin_index.size - 1) // S.TILE * S.TILE
    free = np.flatnonzero((bin2[last:] != 255) & (j[last:] != 0))
    e2 = last + int(free[free.size // 2])
    bin2[e2] = 255
    ac2 = np.insert(ac2, int(np.searchsorted(pos(bin2), e2)), np.float32(0.125))
    assert ac2.size == c.cnt and not np.array_equal(S.tile_counts(bin2), S.tile_counts(c.bin_index))
    m = O.Compressed()
    for k in O.Compressed.__slots__:
        setattr(m, k, getattr(c, k, None))
    m.bin_index, m.ac_exact, m.cnt = bin2, ac2, ac2.size
    return bin2, ac2, O.decompress(m, O.FAST)


def test_time_steps_memo_pair_on_the_chain(delay):
    """MEMO_PAIR rotated through one buffer on the chain of kernels: every decode starts from the memo (counter 16); where
    the stream buffers are rewritten behind the compress call, it is found stale and decoded again (counter 17)."""
    n = S.SUBJECTS[S.MEMO_PAIR[0]].n
    st = Steps(delay, n, S.F64)
    try:
        ctx = st.ctx
        ctx.set_one_launch(False)
        for i in range(8):
            name = S.MEMO_PAIR[i % 2]
            c = S.streams(name)
            m0, r0 = ctx.counter(MEMO), ctx.counter(REDO)
            info, got = st.compress(name, S.SUBJECTS[name].x, O.EC)
            if i % 4 >= 2:                                # the streams are rewritten between the two calls
                bin2, ac2, want = _flag_moved(c)
                rec = st.decompress(info, O.EC, rewrite=[("bin_index", st.dev((name, "bin2"), bin2)), ("ac_exact", st.dev((name, "ac2"), ac2))])
            else:
                want = S.decode(name)
                rec = st.decompress(info, O.EC)
            _check_streams(f"step {i}", info, got, c)
            assert _same(rec.cpu().numpy(), want), f"step {i}: the decode of {name} differs"
            assert not ctx.last_kernel(0).startswith("k_compress_one")
            assert ctx.counter(MEMO) == m0 + 1, f"step {i}"
            assert ctx.counter(REDO) == r0 + (1 if i % 4 >= 2 else 0), f"step {i}"
    finally:
        st.close()


def test_time_steps_qt_pair(delay):
    """QT_PAIR rotated through one buffer (the one-launch kernels): the tables of a step never reach the next."""
    n = S.SUBJECTS[S.QT_PAIR[0]].n
    st = Steps(delay, n, S.F64)
    try:
        for i in range(6):
            name = S.QT_PAIR[i % 2]
            calls = st.ctx.counter(ONE_CALLS)
            info, got = st.compress(name, S.SUBJECTS[name].x, O.QT)
            rec = st.decompress(info, O.QT)
            _check_streams(f"step {i}", info, got, S.streams(name))
            assert _same(rec.cpu().numpy(), S.decode(name)), f"step {i}: the decode of {name} differs"
            assert st.ctx.counter(ONE_CALLS) == calls + 2
    finally:
        st.close()


def test_time_steps_remembered_sf_across_a_decade(delay):
    """`big`, `big` two decades up and `big` again through one buffer, with set_speculation(True, 1 << 18) on the chain: the
    guess comes from the remembered statistics from the third call (counter 18) and is wrong at the change of decade
    (counter 19) -- the streams are the oracle's at every step."""
    big, up = S.SUBJECTS["big"], S.BIG_UP
    cs = {"big": S.streams("big"), "big_up": O.compress(up.x, S.EB, O.EC, O.FAST)}
    want = {"big": S.decode("big"), "big_up": O.decompress(cs["big_up"], O.FAST)}
    assert cs["big_up"].sf == 100.0 * cs["big"].sf
    st = Steps(delay, big.n, S.F64)
    try:
        ctx = st.ctx
        ctx.set_one_launch(False)
        ctx.set_speculation(True, S.SPEC_MIN)
        order = ["big"] * 4 + ["big_up"] * 2 + ["big"] * 2
        for i, name in enumerate(order):
            hits, hist, miss = ctx.counter(SPEC_HITS), ctx.counter(HIST_HITS), ctx.counter(HIST_MISSES)
            info, got = st.compress(name, (big if name == "big" else up).x, O.EC)
            rec = st.decompress(info, O.EC)
            _check_streams(f"step {i}", info, got, cs[name])
            assert _same(rec.cpu().numpy(), want[name]), f"step {i}: the decode of {name} differs"
            if i < 4:
                assert ctx.counter(SPEC_HITS) == hits + 1, i
                assert ctx.counter(HIST_HITS) == hist + (1 if i >= 2 else 0), i
                assert ctx.counter(HIST_MISSES) == miss, i
            elif i == 4:
                assert ctx.counter(HIST_MISSES) == miss + 1 and ctx.counter(HIST_HITS) == hist, "the change of decade"
    finally:
        st.close()


# ---- entry points outside the vocabulary --------------------------------------------------------------------------------------
class Raw:
    """One context for raw C calls on one input buffer that holds a decoy until the delay is over."""

    def __init__(self, delay, name):
        import torch
        import dctz_amd
        self.torch, self.s = torch, S.SUBJECTS[name]
        self.ctx = dctz_amd.Context(0)
        self.gate = Gate(self.ctx, delay)
        self.x = np.ascontiguousarray(self.s.x.reshape(-1))
        self.true = torch.from_numpy(self.x.copy()).to(self.ctx.device)
        self.xin = torch.empty_like(self.true)
        self.dt = H.F64 if self.s.dtype == S.F64 else H.F32

    def enter(self):
        _decoy(self.xin)
        self.gate.arm(lambda: [(self.xin, self.true)])
        self.ctx._bind_stream()
        assert self.gate.disarm() == 1

    def recycle(self):
        _decoy(self.xin)

    def close(self):
        self.torch.cuda.synchronize()
        pending = self.gate.pending
        TALLY["work ops"] += len(pending)
        TALLY["pending at entry"] += sum(pending)
        self.ctx.close()
        assert all(pending)


@pytest.fixture()
def raw(delay, request):
    r = Raw(delay, request.param)
    yield r
    r.close()


SMALL = ["a2597", "c12288", "t2r", "t3r"]


@pytest.mark.parametrize("raw", SMALL, indirect=True)
def test_stats_behind_a_pending_producer(raw):
    x, c = raw.x, S.streams(raw.s.name)
    st = H.CompressInfo()
    raw.enter()
    rc = raw.ctx.lib.dctzhip_stats(raw.ctx.h, raw.xin.data_ptr(), x.size, raw.dt, C.byref(st))
    raw.recycle()
    assert rc == 0
    a = np.abs(x)
    assert (st.max_abs, st.min_abs) == (float(a.max()), float(a.min())) and st.nblk == (x.size + 63) // 64
    if raw.s.flat:
        assert st.sf == c.sf
    mean = math.fsum(x[1:].tolist()) / x.size
    assert abs(st.mean - mean) <= 1e-5 * max(1.0, abs(mean)), (st.mean, mean)       # (tests/test_gpu_parity.py's rule)


@pytest.mark.parametrize("raw", SMALL, indirect=True)
def test_serial_mean_behind_a_pending_producer(raw):
    """begin() on the side stream sums the TRUE data, in serial order: numpy's cumulative sum runs in that order."""
    x, T = raw.x, raw.s.dtype.type
    mean = C.c_double(0.0)
    raw.enter()
    rc = raw.ctx.lib.dctzhip_serial_mean_begin(raw.ctx.h, raw.xin.data_ptr(), x.size, raw.dt)
    rc2 = raw.ctx.lib.dctzhip_serial_mean_end(raw.ctx.h, C.byref(mean))
    raw.recycle()
    assert rc == 0 and rc2 == 0
    want = np.cumsum(x[1:], dtype=T)[-1] / T(x.size)
    assert mean.value == float(want), (mean.value, float(want))


@pytest.mark.parametrize("raw", ["a2597", "c12288"], indirect=True)
def test_scale_inplace_behind_a_pending_producer(raw):
    x, c = raw.x, S.streams(raw.s.name)
    assert c.sf != 1.0
    raw.enter()
    rc = raw.ctx.lib.dctzhip_scale_inplace(raw.ctx.h, raw.xin.data_ptr(), x.size, raw.dt, float(c.sf))
    got = raw.xin.clone()
    raw.recycle()
    assert rc == 0
    assert _same(got.cpu().numpy(), x / raw.s.dtype.type(c.sf)) and _same(got.cpu().numpy(), c.scaled)


@pytest.mark.parametrize("raw", ["a2597", "c12288"], indirect=True)
def test_compress_part_behind_a_pending_producer(raw):
    """Two parts of one subject, each entered with the part's input pending; the streams are the one call's."""
    x, c, ctx = raw.x, S.streams(raw.s.name), raw.ctx
    n = x.size
    out = ctx.alloc_outputs(n)
    for v in out.values():
        v.view(raw.torch.uint8).fill_(FILL)
    cut = (n // 64 * 2 // 3) * 64
    mx, mn = float(np.abs(x).max()), float(np.abs(x).min())
    at, total = 0, 0.0
    for lo, hi in ((0, cut), (cut, n)):
        _decoy(raw.xin)
        raw.gate.arm(lambda: [(raw.xin, raw.true)])
        cnt, st, sf = ctx.compress_part(raw.xin[lo:hi], S.EB, mx, mn, out, lo, at)
        assert raw.gate.disarm() == 1
        got = {k: v.clone() for k, v in out.items()}
        raw.recycle()
        assert sf == c.sf and st[0] == float(np.abs(x[lo:hi]).max()) and st[1] == float(np.abs(x[lo:hi]).min())
        total += st[2] + (float(x[lo]) if lo else 0.0)
        at += cnt
    assert at == c.cnt
    assert _same(got["bin_index"].cpu().numpy(), c.bin_index) and _same(got["dc"].cpu().numpy(), c.dc)
    assert _same(got["ac_exact"][:at].cpu().numpy(), c.ac_exact)
    assert int((got["ac_exact"][at:].view(raw.torch.uint8) != FILL).sum().item()) == 0
    mean = math.fsum(x[1:].tolist()) / n
    assert abs(total / n - mean) <= 1e-5 * max(1.0, abs(mean))
