"""Placement ("Placement, what is pinned"): every device buffer a call receives starts at the weakest
alignment include/dctz_hip.h allows its role -- at `a` past a multiple of 256 bytes (PAST) or at `a` before one (BEFORE).

The other GPU tests pass torch allocations and arena cuts at multiples of 256: a kernel that assumes a 32-, 64- or 128-byte
base, a host path that rounds a pointer, a reduction whose tree peels to an aligned address all pass there.  Here the
runner of the call-order tests plays the fixed schedules of tests/placement_cases.py with its subjects' inputs, the indices, the
stream slots (the ones compress writes at 16, decode-only copies of the oracle's streams with DC and AC_exact at 4), the lists,
masks and records an op uploads and every output -- the wrapper's own allocations included -- cut from 0xA5 arenas at the
residue of their role; the guards stay at least 256 bytes and are checked after every op.  Expected values are the runner's
own: E1 the oracle and the numpy models, E2 a fresh context on DEFAULT-aligned buffers, so a result that moves with placement
fails.  A proxy around the context's library asserts the residue of every device pointer of every work call."""
import ctypes as C
import math

import numpy as np
import pytest

from dctz_amd import hip as H
from tests import placement_cases as P
from tests import sequence_cases as S
from tests.sequence_runner import FILL, Arena, Runner, _e2

pytestmark = pytest.mark.gpu


class PlacedArena(Arena):
    """An arena whose cuts start at the residue of their role under the runner's placement."""

    def __init__(self, device, nbytes, runner):
        super().__init__(device, nbytes)
        self.runner = runner

    def take(self, shape, dtype, align=None, role=None):
        R = self.runner
        esize = R.torch.empty(0, dtype=dtype).element_size()
        if role is None:
            role = P.alloc_role(R.kind, str(dtype).split(".")[-1])
        res = P.residue(role, esize, R.next_placement())
        t = super().take(shape, dtype, align=res)
        assert t.data_ptr() % P.LINE == res
        return t

    def holds(self, p):
        return self.base <= p < self.base + self.buf.numel()


class Proxy:
    """What the context sees as its library: every work call's device pointers are checked before the call is made."""

    def __init__(self, lib, runner):
        self._lib, self._runner = lib, runner

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in P.ROLES and name not in P.TABLES and name not in P.ALLOW:
            return f
        R = self._runner

        def checked(*args):
            R.calls.append(name)
            for i, role in zip(P.pointer_positions(name), P.ROLES.get(name, ())):
                v = args[i] if i < len(args) else None
                v = v.value if isinstance(v, C.c_void_p) else v
                if v is not None:
                    R.check_pointer(f"{name}, argument {i}", int(v), role)
            if name in P.TABLES:
                at_k, at_items, item, fields = P.TABLES[name]
                items = C.cast(args[at_items], C.POINTER(item))
                for j in range(int(args[at_k])):
                    for field, role in fields.items():
                        v = getattr(items[j], field)
                        if v:
                            R.check_pointer(f"{name}, item {j}.{field}", int(v), role, table=True)
            return f(*args)
        return checked


class PlacementRunner(Runner):
    def __init__(self, placement, **kw):
        self.placement, self.kind, self.esize = placement, "", 8
        self.flip, self.calls, self.seen, self.table_placements, self.loose = 0, [], [], set(), False
        super().__init__(persistent=40 << 20, transient=24 << 20, **kw)
        self.ctx.lib = Proxy(self.ctx.lib, self)
        self.dec = {}

    def _arena(self, nbytes):
        return PlacedArena(self.ctx.device, nbytes, self)

    def next_placement(self):
        if self.placement != P.MIXED:
            return self.placement
        self.flip += 1
        return P.PLACEMENTS[self.flip % 2]

    def check_pointer(self, what, p, role, table=False):
        inside = self.keep.holds(p) or self.tmp.holds(p)
        if role == P.HOST:
            assert not inside, f"{what}: a host pointer inside an arena"
            return
        assert inside, f"{what}: device pointer {p:#x} lies outside the arenas"
        if role == P.ANY or self.loose:
            return
        want = [P.residue(role, self.esize, pl) for pl in (P.PLACEMENTS if self.placement == P.MIXED else (self.placement,))]
        assert p % P.LINE in want, f"{what}: {p:#x} is at {p % P.LINE} (mod 256), its role ({role}) under '{self.placement}' asks {want}"
        self.seen.append((what, p % P.LINE))
        if table:
            self.table_placements.add(P.PLACEMENTS[want.index(p % P.LINE)] if self.placement == P.MIXED else self.placement)

    # ---- device copies: from the persistent arena, at the residue of their role ----
    def _upload(self, a, role):
        return self.keep.put(a, role=role)

    def x(self, name, raw=False):
        if self.kind != "summary_nd_ref":
            return super().x(name, raw)
        key = (name, raw, P.ES)                               # the original of tile_summary_nd: aligned to its elements
        if key not in self.inputs:
            s = S.SUBJECTS[name]
            self.inputs[key] = self._upload(s.raw if raw else s.x, P.ES)
        return self.inputs[key]

    def slot(self, slot, name, for_decode=False):
        if not for_decode:
            return super().slot(slot, name)
        if name not in self.dec:                              # decode-only copies of the oracle's streams: DC, AC_exact at 4
            c = S.streams(name)
            ac = c.ac_exact if c.cnt else np.zeros(1, np.float32)
            self.dec[name] = {"bin_index": self.keep.put(c.bin_index, role=16), "dc": self.keep.put(c.dc, role=4), "ac_exact": self.keep.put(ac, role=4)}
        return self.dec[name]

    def launch(self, op, where=""):
        self.kind = op[0]
        names = S.targets(*op) if op[0] in S.OPS else []
        if names:
            self.esize = S.SUBJECTS[names[0]].dtype.itemsize
        self.calls, before = [], len(self.seen)
        super().launch(op, where)
        if op[0] in S.OPS:
            missing = [f for f in P.KIND_CALLS[op[0]] if f not in self.calls]
            assert not missing, f"{where}: {op[0]} never called {missing} through the checked library"
            assert len(self.seen) > before or all(f in P.ALLOW for f in P.KIND_CALLS[op[0]]), f"{where}: no device pointer was checked"


def _play(placement, sched, where):
    r = PlacementRunner(placement, e2=_e2)
    ran = 0
    try:
        for i, op in enumerate(sched):
            r.run(op, f"{where}, op {i}")
            ran += 1
        work = sum(1 for k, _, _ in sched if k in S.OPS)
        print(f"{where}: {work} work ops, {len(r.seen)} device pointers at their residue")
    finally:
        r.close()
    assert ran == len(sched), "the runner leaves no op out"
    return r.table_placements


SCHEDULES = P.schedules()


@pytest.mark.parametrize("placement", P.PLACEMENTS)
@pytest.mark.parametrize("family", list(SCHEDULES))
def test_family_at_the_weakest_alignment(family, placement):
    _play(placement, SCHEDULES[family], f"{family} / {placement}")


def test_batches_with_members_of_both_placements():
    """The buffers alternate between PAST and BEFORE, so every batch call holds members of both."""
    lists = [op for op in SCHEDULES["box"] + SCHEDULES["coarse"] if op[0] in ("boxes", "boxes_nd", "coarse_boxes_nd")]
    sched = SCHEDULES["batch"] + lists[:4] + lists[-6:]
    assert _play(P.MIXED, sched, "batch / mixed") == set(P.PLACEMENTS)


# ---- entry points outside the vocabulary, as tests/test_gpu_stream_order.py calls them -------------------------------------------
@pytest.fixture(params=[(n, pl) for n in P.RAW_SUBJECTS for pl in P.PLACEMENTS], ids=lambda v: f"{v[0]}-{v[1]}")
def raw(request):
    name, placement = request.param
    r = PlacementRunner(placement)
    r.kind, r.esize = "raw", S.SUBJECTS[name].dtype.itemsize
    s = S.SUBJECTS[name]
    yield r, s, np.ascontiguousarray(s.x.reshape(-1)), H.F64 if s.dtype == S.F64 else H.F32
    bad = int(r.tmp.damaged().item()) + int(r.keep.damaged().item())
    r.close()
    assert bad == 0, f"{bad} bytes outside the buffers were written"


def test_stats_and_serial_mean(raw):
    r, s, x, dt = raw
    xd, c = r.keep.put(x, role=16), S.streams(s.name)
    st = H.CompressInfo()
    assert r.ctx.lib.dctzhip_stats(r.ctx.h, xd.data_ptr(), x.size, dt, C.byref(st)) == 0
    a = np.abs(x)
    assert (st.max_abs, st.min_abs, st.sf) == (float(a.max()), float(a.min()), c.sf) and st.nblk == (x.size + 63) // 64
    mean = math.fsum(x[1:].tolist()) / x.size
    assert abs(st.mean - mean) <= 1e-5 * max(1.0, abs(mean)), (st.mean, mean)         # (tests/test_gpu_parity.py's rule)
    got = C.c_double(0.0)
    assert r.ctx.lib.dctzhip_serial_mean_begin(r.ctx.h, xd.data_ptr(), x.size, dt) == 0
    assert r.ctx.lib.dctzhip_serial_mean_end(r.ctx.h, C.byref(got)) == 0
    T = s.dtype.type
    assert got.value == float(np.cumsum(x[1:], dtype=T)[-1] / T(x.size))
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), x.view(np.uint8))
    assert r.calls == ["dctzhip_stats", "dctzhip_serial_mean_begin"] and len(r.seen) == 2


def test_scale_inplace(raw):
    r, s, x, dt = raw
    xd, c = r.keep.put(x, role=16), S.streams(s.name)
    assert c.sf != 1.0
    assert r.ctx.lib.dctzhip_scale_inplace(r.ctx.h, xd.data_ptr(), x.size, dt, float(c.sf)) == 0
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), c.scaled.view(np.uint8)) and len(r.seen) == 1


def test_compress_part(raw):
    """Two parts of one subject: the part's streams go to bin_index + lo (16), DC + lo / 64 and AC_exact + ac_at (4 bytes each)."""
    r, s, x, dt = raw
    c, n, t = S.streams(s.name), x.size, r.torch
    xd = r.keep.put(x, role=16)
    out = {"bin_index": r.keep.take(n, t.uint8, role=16), "dc": r.keep.take((n + 63) // 64, t.float32, role=4), "ac_exact": r.keep.take(n, t.float32, role=4)}
    cut = (n // 64 * 2 // 3) * 64
    mx, mn = float(np.abs(x).max()), float(np.abs(x).min())
    at = 0
    for lo, hi in ((0, cut), (cut, n)):
        r.loose = lo != 0                                 # (the second part's pointers are the first's plus lo, lo / 16 and 4 ac_at:
        cnt, st, sf = r.ctx.compress_part(xd[lo:hi], S.EB, mx, mn, out, lo, at)     # inside the arenas, wherever that is)
        assert sf == c.sf and st[0] == float(np.abs(x[lo:hi]).max()) and st[1] == float(np.abs(x[lo:hi]).min())
        at += cnt
    assert at == c.cnt
    same = lambda g, w: np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))    # noqa: E731
    assert same(out["bin_index"], c.bin_index) and same(out["dc"], c.dc) and same(out["ac_exact"][:at], c.ac_exact)
    assert int((out["ac_exact"][at:].view(t.uint8) != FILL).sum().item()) == 0
    assert r.calls == ["dctzhip_compress_part"] * 2
