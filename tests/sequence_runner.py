"""The runner of the call-order and stream-order tests ("Call order" and "Stream order"): one context,
its 0xA5 arenas with guard bands, the device copies of the subjects of tests/sequence_cases.py, one implementation per op
kind (_IMPL) whose results come back as a list of checks (label, got, expected), and E2 -- every (op, subject) as the first
work call of a fresh context on an idle stream, once per process.  tests/test_gpu_call_sequences.py plays schedules on it as
it is; tests/test_gpu_stream_order.py on a subclass that keeps the stream busy around every call."""
import ctypes as C

import numpy as np

from dctz_amd import hip as H
from oracle import oracle as O
from tests import sequence_cases as S

GUARD = 256
FILL = 0xA5
ONE_CALLS, ONE_GAVE_UP, SPEC_HITS, MEMO, HIST_HITS, VARIANT = 0, 1, 6, 16, 18, 20      # dctzhip_debug_counter
E2 = object()                           # in a check: the expected value is the fresh context's


class E2Of:
    """In a check: the expected value is fn(the fresh context's result `label` of ANOTHER op) -- a slice taken on the host."""

    def __init__(self, op, label, fn):
        self.op, self.label, self.fn = op, label, fn


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _up(n):
    return (int(n) + GUARD - 1) // GUARD * GUARD


class Arena:
    """A device buffer of 0xA5 bytes that outputs are cut from, each 256-byte aligned (or at `align` bytes past a multiple of
    256: take(..., align=a), 0 <= a < 256) with at least 256 bytes of guard on either side."""

    def __init__(self, device, nbytes):
        import torch
        self.buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.top = 0
        self.live = []                  # (start, nbytes) of every output cut since the last reset

    def take(self, shape, dtype, align=256, role=None):         # role: what the buffer is for (tests/placement_cases.py)
        import torch
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        esize = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esize
        assert self.base % GUARD == 0 and 0 <= align % GUARD < GUARD and (align % GUARD) % esize == 0
        start = self.top + GUARD + align % GUARD         # (top is a multiple of 256, and so is the arena's own address)
        assert _up(start + nbytes) + GUARD <= self.buf.numel(), "arena too small"
        self.top = _up(start + nbytes)
        self.live.append((start, nbytes))
        return self.buf[start:start + nbytes].view(dtype).view(shape)

    def put(self, a, align=256, role=None):
        import torch
        t = torch.from_numpy(np.array(a, copy=True, order="C"))
        d = self.take(tuple(t.shape), t.dtype, align, role)
        d.copy_(t)
        return d

    def damaged(self):
        """Bytes that are not 0xA5 in the guards of the live outputs and in the space no output was cut from (a tensor)."""
        parts = [self.buf[self.top:]]
        for start, nbytes in self.live:
            parts += [self.buf[start - GUARD - start % GUARD:start], self.buf[start + nbytes:_up(start + nbytes)]]
        import torch
        return (torch.cat(parts) != FILL).sum()

    def reset(self):
        if self.top:
            self.buf[:self.top].fill_(FILL)
        self.top, self.live = 0, []


class _ArenaTorch:
    """What the wrapper sees as `torch`: its output allocations come from the arena, everything else is torch's."""

    def __init__(self, arena):
        import torch
        self._arena, self._torch = arena, torch

    def __getattr__(self, k):
        return getattr(self._torch, k)

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, self._torch.Size)):
            shape = tuple(shape[0])
        return self._arena.take(shape, dtype)

    def empty_like(self, x):
        return self._arena.take(tuple(x.shape), x.dtype)


class Mismatch(AssertionError):
    pass


class Runner:
    """One context, its arenas, the device copies of the subjects and the buffers their streams live in."""

    def __init__(self, e2=None, record=None, stream=None, persistent=12 << 20, transient=20 << 20):
        import torch
        import dctz_amd
        self.torch = torch
        self.stream = stream
        with self._on_stream():
            self.ctx = dctz_amd.Context(0)
            self.keep = self._arena(persistent)                   # the slots: outputs that stay for later ops
            self.tmp = self._arena(transient)                     # the outputs of one op
        self.ctx.torch = _ArenaTorch(self.tmp)
        self.e2, self.record = e2, record
        self.slots, self.holder, self.inputs, self.indices = {}, {}, {}, {}
        self.pending = None
        self.trace = []

    def _arena(self, nbytes):
        return Arena(self.ctx.device, nbytes)

    def _upload(self, a, role):
        """A device copy of a subject's array or index (a torch allocation; the placement runner cuts it from an arena)."""
        return self.torch.from_numpy(np.array(a, copy=True)).to(self.ctx.device)

    def _on_stream(self):
        import contextlib
        return self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def close(self):
        self.ctx.close()

    # ---- device copies ----
    def x(self, name, raw=False):
        key = (name, raw)
        if key not in self.inputs:
            s = S.SUBJECTS[name]
            self.inputs[key] = self._upload(s.raw if raw else s.x, 16)
        return self.inputs[key]

    def index(self, name):
        if name not in self.indices:
            self.indices[name] = self._upload(S.index(name), 4)
        return self.indices[name]

    def slot(self, slot, name, for_decode=False):
        """The stream buffers `slot` (by default one per subject, holding the oracle's streams until a compress writes them)."""
        s = S.SUBJECTS[name]
        if slot not in self.slots:
            t = self.torch
            self.slots[slot] = {"bin_index": self.keep.take(s.n_lin, t.uint8), "dc": self.keep.take(s.n_lin // 64 + (s.n_lin % 64 != 0), t.float32),
                                "ac_exact": self.keep.take(s.n_lin, t.float32)}
            self.holder[slot] = None
            if slot == name:
                c = S.streams(name)
                b = self.slots[slot]
                b["bin_index"].copy_(t.from_numpy(c.bin_index.copy()))
                b["dc"].copy_(t.from_numpy(c.dc.copy()))
                b["ac_exact"][:c.cnt].copy_(t.from_numpy(c.ac_exact.copy()))
                self.holder[slot] = name
        assert self.slots[slot]["bin_index"].numel() == s.n_lin
        if for_decode:
            assert self.holder[slot] == name, f"schedule error: slot {slot} holds {self.holder[slot]}, not {name}"
        return self.slots[slot]

    def poison(self, b):
        for v in b.values():
            v.view(self.torch.uint8).fill_(FILL)

    # ---- one op ----
    def launch(self, op, where=""):
        kind, name, args = op
        with self._on_stream():
            try:
                checks = _IMPL[kind](self, kind, name, {k: v for k, v in args.items() if k != "ctx"})
            except H.DctzHipError as e:
                raise Mismatch(f"{where}: the call was refused -- {e}\n{self._context(op)}") from e
            self.pending = (op, checks)

    def finish(self, where=""):
        op, checks = self.pending
        self.pending = None
        with self._on_stream():
            for label, got, want in checks:
                self._compare(where, op, label, got, want)
            bad = int(self.tmp.damaged().item()) + int(self.keep.damaged().item())
            if bad:
                raise Mismatch(f"{where}: {bad} bytes outside the outputs were written (guard bands / free arena)\n{self._context(op)}")
            self.tmp.reset()
        self.trace.append(op)

    def run(self, op, where=""):
        self.launch(op, where)
        self.finish(where)

    def _context(self, op):
        return "  op: %r\n  previous: %s" % (op, "\n            ".join(repr(o) for o in self.trace[-5:]))

    @staticmethod
    def _host(v):
        if callable(v):
            v = v()
        if hasattr(v, "is_cuda"):
            v = v.contiguous().cpu().numpy()
        if isinstance(v, (list, tuple)) and not isinstance(v, np.ndarray):
            v = np.array(v)
        return np.ascontiguousarray(v)

    def _compare(self, where, op, label, got, want):
        got = self._host(got)
        if want is E2:
            key = S.e2_key(op[0], op[1], op[2]) + (label,)
            if self.record is not None:
                self.record[key] = got.copy()
                return
            want = self.e2(op)[key]
        elif isinstance(want, E2Of):
            if self.record is not None:                  # (a fresh context's own result: two of them are compared once)
                self.record[S.e2_key(op[0], op[1], op[2]) + (label,)] = got.copy()
                return
            want = want.fn(self.e2(want.op)[S.e2_key(*want.op) + (want.label,)])
        want = self._host(want)
        g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
        if got.size == want.size and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(g, w):
            return
        if got.size != want.size or got.dtype.itemsize != want.dtype.itemsize:
            detail = f"{got.size} x {got.dtype} against {want.size} x {want.dtype}"
        else:
            i = int(np.flatnonzero(g != w)[0]) // got.dtype.itemsize
            detail = f"first difference at element {i} of {got.size}: got {got.reshape(-1)[i]!r}, expected {want.reshape(-1)[i]!r}"
        raise Mismatch(f"{where}: '{label}' differs -- {detail}\n{self._context(op)}")


# ---- the ops --------------------------------------------------------------------------------------------------------------
def _q(c, s):
    return c.qtable if s.mode == O.QT else None


def _stream_checks(R, b, info, c, s, pre=""):
    t = R.torch
    n_ac = b["ac_exact"].numel()
    checks = [(pre + "sf", info.sf, c.sf), (pre + "cnt", int(info.cnt), int(c.cnt)), (pre + "bin_index", b["bin_index"], c.bin_index),
              (pre + "dc", b["dc"], c.dc), (pre + "ac_exact", b["ac_exact"][:c.cnt], c.ac_exact),
              (pre + "ac_exact beyond cnt", lambda: int((b["ac_exact"][c.cnt:].view(t.uint8) != FILL).sum().item()) if n_ac > c.cnt else 0, 0)]
    if c.mode == O.QT:
        checks += [(pre + "qtable", np.array(info.qtable[:], dtype=s.dtype), c.qtable), (pre + "qtable_raw", np.array(info.qtable_raw[:], dtype=s.dtype), c.qtable_raw)]
    return checks


def _compress(R, kind, name, a):
    s, c = S.SUBJECTS[name], S.streams(name)
    slot = a.get("slot", name)
    b = R.slot(slot, name)
    R.poison(b)
    xd, kw = R.x(name), {}
    if kind == "compress_scaled":
        kw["scaled"] = R.tmp.take(s.n, _tdt(s.dtype))
    elif kind == "compress_inplace":
        xd = R.tmp.put(s.x)
        kw["scaled"] = xd
    elif kind == "compress_coef":
        kw["coef"] = R.tmp.take(s.n, _tdt(s.dtype))
    _, info = R.ctx.compress(xd, S.EB, s.mode, out=b, **kw)
    R.holder[slot] = name
    checks = _stream_checks(R, b, info, c, s) + [("variant", R.ctx.counter(VARIANT), S.variant(name))]
    if "scaled" in kw:
        checks.append(("scaled", kw["scaled"], c.scaled))
    if "coef" in kw:
        checks.append(("coef", kw["coef"], c.coef if s.mode == O.EC else E2))     # (QT: the oracle's array holds the normalised values)
    return checks


def _decode_args(R, name, a):
    s, c = S.SUBJECTS[name], S.streams(name)
    return s, c, R.slot(a.get("slot", name), name, for_decode=True), _tdt(s.dtype)


def _decompress(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    return [("decode", R.ctx.decompress(b, c.cnt, s.n, tdt, S.EB, c.sf, s.mode, qtable=_q(c, s)), S.decode(name))]


def _compress_nd(R, kind, name, a):
    s, c = S.SUBJECTS[name], S.streams(name)
    b = R.slot(name, name)
    R.poison(b)
    _, info = R.ctx.compress_nd(R.x(name), S.EB, s.mode, out=b)
    R.holder[name] = name
    return _stream_checks(R, b, info, c, s) + [("variant", R.ctx.counter(VARIANT), S.variant(name))]


def _decompress_nd(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    return [("decode", R.ctx.decompress_nd(b, c.cnt, s.shape, tdt, S.EB, c.sf, s.mode, qtable=_q(c, s)), S.decode(name))]


def _range(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    idx, tot = R.ctx.ac_index(b, s.n)
    r = R.ctx.decompress_range(b, c.cnt, s.n, tdt, S.EB, c.sf, a["lo"], a["hi"], idx, s.mode, qtable=_q(c, s))
    return [("index", idx, S.index(name)), ("index total", tot, int(c.cnt)), ("range", r, S.decode(name)[a["lo"]:a["hi"]])]


def _box(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    nd = kind.endswith("_nd")
    shape = s.shape if nd else s.dims
    if kind.startswith("boxes"):
        f = R.ctx.decompress_boxes_nd if nd else R.ctx.decompress_boxes
        rs = f(b, c.cnt, shape, tdt, S.EB, c.sf, [tuple(bx) for bx in a["boxes"]], R.index(name), s.mode, qtable=_q(c, s))
        return [(f"box {i}", r, S.box_of(name, lo, hi, nd)) for i, (r, (lo, hi)) in enumerate(zip(rs, a["boxes"]))]
    f = R.ctx.decompress_box_nd if nd else R.ctx.decompress_box
    r = f(b, c.cnt, shape, tdt, S.EB, c.sf, a["lo"], a["hi"], R.index(name), s.mode, qtable=_q(c, s))
    return [("box", r, S.box_of(name, a["lo"], a["hi"], nd))]


def _coarse(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    if s.flat:
        r = R.ctx.decompress_coarse(b, c.cnt, s.n, tdt, S.EB, c.sf, a["factor"], index=R.index(name), mode=s.mode, qtable=_q(c, s))
    else:
        r = R.ctx.decompress_coarse_nd(b, c.cnt, s.shape, tdt, S.EB, c.sf, a["factor"], index=R.index(name), mode=s.mode, qtable=_q(c, s))
    return [("coarse", r, E2)]


def _coarse_box(R, kind, name, a):
    """A box, or a list of boxes, of the coarse array: the slices of the whole-array op's fresh-context result."""
    s, c, b, tdt = _decode_args(R, name, a)
    f = a["factor"]
    whole = (("coarse_nd", name, {"factor": f}), "coarse")
    ext = S.coarse_shape(s.shape, f)

    def cut(lo, hi):
        return lambda v: np.ascontiguousarray(v.reshape(ext)[tuple(slice(l, h) for l, h in zip(lo, hi))])
    if kind == "coarse_boxes_nd":
        rs = R.ctx.decompress_coarse_boxes_nd(b, c.cnt, s.shape, tdt, S.EB, c.sf, f, [tuple(bx) for bx in a["boxes"]], index=R.index(name), mode=s.mode,
                                              qtable=_q(c, s))
        return [(f"coarse box {i}", r, E2Of(*whole, cut(lo, hi))) for i, (r, (lo, hi)) in enumerate(zip(rs, a["boxes"]))]
    r = R.ctx.decompress_coarse_box_nd(b, c.cnt, s.shape, tdt, S.EB, c.sf, f, a["lo"], a["hi"], index=R.index(name), mode=s.mode, qtable=_q(c, s))
    return [("coarse box", r, E2Of(*whole, cut(a["lo"], a["hi"])))]


def _summary(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    ref = R.x(name) if kind.endswith("_ref") else None
    if s.flat:
        recs, total = R.ctx.tile_summary(b, c.cnt, s.n, tdt, S.EB, c.sf, index=R.index(name), mode=s.mode, qtable=_q(c, s), ref=ref)
    else:
        recs, total = R.ctx.tile_summary_nd(b, c.cnt, s.shape, tdt, S.EB, c.sf, index=R.index(name), mode=s.mode, qtable=_q(c, s), ref=ref)
    fields = [f for f, _ in H.TileSummary._fields_]
    if ref is None:                                       # (without an original the last four fields of a record are not defined)
        recs, fields = recs[:, :4], fields[:4]
    return [("records", recs, E2), ("total", np.array([getattr(total, f) for f in fields]), E2)]


def _fixup(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    start_w, off_w, val_w = S.fix_list(name, a["mult"])
    bound = S.fix_bound(name, a["mult"])
    if "apply" in kind:
        fix = (R.tmp.put(start_w.view(np.int32), role=4), R.tmp.put(off_w.view(np.int16), role=2), R.tmp.put(val_w, role="es"), int(off_w.size))
        dst = R.tmp.put(S.decode(name), role="es")
        r = R.ctx.fixup_apply(fix, s.n, tdt, dst) if s.flat else R.ctx.fixup_apply_nd(fix, s.shape, tdt, dst)
        return [("applied", r, S.fix_applied(name, a["mult"]))]
    f = R.ctx.fixup_build if s.flat else R.ctx.fixup_build_nd
    geo = s.n if s.flat else s.shape
    cap = 0 if "count" in kind else None
    start, off, val, count = f(b, c.cnt, geo, tdt, S.EB, c.sf, R.x(name), bound, index=R.index(name), mode=s.mode, qtable=_q(c, s), capacity=cap)
    checks = [("fix_start", start, start_w), ("count", count, int(off_w.size))]
    if cap is None:
        checks += [("fix_off", off, off_w), ("fix_val", val, val_w)]
    return checks


def _mask(R, kind, name, a):
    s = S.SUBJECTS[name]
    words, count, filled = S.mask(name)
    raw = R.x(name, raw=True)
    if kind in ("mask_build", "mask_build_nd"):
        f = R.ctx.mask_build if s.flat else R.ctx.mask_build_nd
        m, k, fd = f(raw, H.MISS_ABS_GE, 0.0, S.LIMIT)
        return [("mask", m, words), ("count", k, count), ("filled", fd, filled), ("input", raw, s.raw)]
    if kind == "mask_apply":
        dst = R.tmp.put(S.decode(name), role="es")
        m = R.tmp.put(words.view(np.int64), role=8)
        if s.flat:
            r = R.ctx.mask_apply(m, s.n, a["fill"], dst)
        else:
            r = R.ctx.mask_apply(m, s.n, a["fill"], dst, dims=list(s.shape), lo=[0] * len(s.shape), hi=list(s.shape))
        return [("masked", r, np.where(s.miss, s.dtype.type(a["fill"]), S.decode(name)))]
    c = S.streams(name)
    b = R.slot(name, name)
    R.poison(b)
    f = R.ctx.compress_masked if s.flat else R.ctx.compress_masked_nd
    _, info, m, k = f(raw, S.EB, H.MISS_ABS_GE, 0.0, S.LIMIT, s.mode, out=b)
    R.holder[name] = name
    return _stream_checks(R, b, info, c, s) + [("mask", m, words), ("count", k, count), ("input", raw, s.raw)]


def _rd(R, kind, name, a):
    s = S.SUBJECTS[name]
    xd = R.x(name)
    if kind.startswith("rd_probe"):
        pts, rng = (R.ctx.rd_probe if s.flat else R.ctx.rd_probe_nd)(xd, list(S.RD_EBS))
        checks = [("range", np.array(rng), E2)]
        for p, eb in zip(pts, S.RD_EBS):
            checks += [(f"cnt at {eb}", int(p["cnt"]), int(S.streams_at(name, eb, O.EC).cnt)),
                       (f"point at {eb}", np.array([p["error_bound"], p["sse"], p["psnr"], float(p["raw_bytes"])]), E2)]
        return checks
    if kind == "psnr_terms":
        return [("terms", np.array(R.ctx.psnr_terms(xd.view(-1), R.tmp.put(S.decode(name)).view(-1))), E2)]
    out, info, eb, ps = (R.ctx.compress_psnr if s.flat else R.ctx.compress_psnr_nd)(xd, S.PSNR_TARGET)
    assert eb in H.psnr_grid()
    return [("bound and psnr", np.array([eb, ps]), E2)] + _stream_checks(R, out, info, S.streams_at(name, eb, O.EC), s)


def _dct(R, kind, name, a):
    return [("dct", R.ctx.dct_blocks(R.x(name), inverse=a["inverse"]), S.dct_of(name, a["inverse"]))]


def _batch(R, kind, name, a):
    members = a["members"]
    slots = a.get("slots", members)
    subs = [S.SUBJECTS[m] for m in members]
    cs = [S.streams(m) for m in members]
    mode = subs[0].mode
    if kind == "compress_batch":
        bs = [R.slot(sl, m) for sl, m in zip(slots, members)]
        for b in bs:
            R.poison(b)
        _, infos, _ = R.ctx.compress_batch([R.x(m) for m in members], S.EB, mode, outs=bs)
        checks = []
        for sl, m, b, info, c, s in zip(slots, members, bs, infos, cs, subs):
            R.holder[sl] = m
            checks += _stream_checks(R, b, info, c, s, pre=f"{m}: ")
        return checks
    bs = [R.slot(sl, m, for_decode=True) for sl, m in zip(slots, members)]
    dsts, status, _ = R.ctx.decompress_batch(bs, [c.cnt for c in cs], [s.n for s in subs], [_tdt(s.dtype) for s in subs], S.EB, [c.sf for c in cs], mode,
                                             qtables=[c.qtable for c in cs] if mode == O.QT else None)
    return [("status", list(status), [0] * len(members))] + [(f"{m}: decode", d, S.decode(m)) for m, d in zip(members, dsts)]


def _deflate(R, kind, name, a):
    s, c, b, tdt = _decode_args(R, name, a)
    want = S.deflated(name)
    raw = [c.bin_index, c.dc, c.ac_exact]
    if kind == "deflate":
        zs, sizes = R.ctx.deflate([b["bin_index"], b["dc"], b["ac_exact"][:c.cnt]], want_index=True)
        checks = []
        for i, (z, sz, (wz, wsz)) in enumerate(zip(zs, sizes, want)):
            checks += [(f"section {i}", z, np.frombuffer(wz, np.uint8)), (f"chunk sizes {i}", np.asarray(sz, np.uint32), np.asarray(wsz, np.uint32))]
        return checks
    zs = [R.tmp.put(np.frombuffer(wz, np.uint8)) for wz, _ in want]
    outs, ok = R.ctx.inflate(zs, [wsz for _, wsz in want], [r.nbytes for r in raw])
    return [("ok", bool(ok), True)] + [(f"section {i}", o, r.view(np.uint8)) for i, (o, r) in enumerate(zip(outs, raw))]


def _state(R, kind, name, a):
    ctx = R.ctx
    if kind in ("one_on", "one_off"):
        ctx.set_one_launch(kind == "one_on")
    elif kind in ("spec_on", "spec_off"):
        ctx.set_speculation(kind == "spec_on", S.SPEC_MIN)
    elif kind in ("specmem_on", "specmem_off"):
        ctx.set_spec_memory(kind == "specmem_on")
    elif kind in ("memo_on", "memo_off"):
        ctx.set_decode_memo(kind == "memo_on")
    elif kind in ("split_on", "split_off"):
        ctx.set_split(1 if kind == "split_on" else 0)
    elif kind == "set_stream":
        ctx._bind_stream()
        assert ctx.lib.dctzhip_set_stream(ctx.h, C.c_void_p(ctx._bound)) == 0
    elif kind == "cooldown":
        ctx.knob(2, a["calls"])
    elif kind == "epoch":
        ctx.knob(4, a["value"])
    else:                                                 # "withheld": exactly what test_gpu_one_fallback.py does, for one call
        gave_up = ctx.counter(ONE_GAVE_UP)
        ctx.knob(0, 1)
        try:
            checks = (_compress if a["call"] == "compress" else _decompress)(R, a["call"], name, {})
        finally:
            ctx.knob(0, 0)
        return checks + [("launches that gave up", lambda: ctx.counter(ONE_GAVE_UP) in (gave_up, gave_up + 1), True)]
    return []


def _refusal(R, kind, name, a):
    ctx, lib = R.ctx, R.ctx.lib
    ctx._bind_stream()
    if kind == "ref_sections":
        t = R.tmp.take(64, R.torch.uint8)
        z = R.tmp.take(1024, R.torch.uint8)
        k = 9
        rc = lib.dctzhip_deflate(ctx.h, k, (C.c_void_p * k)(*[t.data_ptr()] * k), (C.c_size_t * k)(*[64] * k), (C.c_void_p * k)(*[z.data_ptr()] * k),
                                 (C.c_size_t * k)(*[1024] * k), (C.c_size_t * k)(), None)
        return [("code", rc, S.REFUSALS[kind])]
    s, c, b, tdt = _decode_args(R, name, a)
    if kind == "ref_space":
        want = S.fix_list(name, a["mult"])
        try:
            ctx.fixup_build(b, c.cnt, s.n, tdt, S.EB, c.sf, R.x(name), S.fix_bound(name, a["mult"]), index=R.index(name), mode=s.mode, qtable=_q(c, s),
                            capacity=int(want[1].size) - 1)
        except H.DctzHipError as e:
            return [("code", f"({H.E_SPACE})" in str(e), True), ("count", int(e.count), int(want[1].size))]
        return [("code", 0, S.REFUSALS[kind])]
    dst = R.tmp.take(s.n + 4, tdt)
    q = ctx._qtable(s.mode, _q(c, s), tdt)
    lo, hi, out = 0, s.n, dst.data_ptr()
    if kind == "ref_null":
        out = None
    elif kind == "ref_misaligned":
        out += 4
    else:
        lo = hi = s.n
    rc = lib.dctzhip_decompress_range(ctx.h, b["bin_index"].data_ptr(), b["dc"].data_ptr(), b["ac_exact"].data_ptr(), int(c.cnt), R.index(name).data_ptr(),
                                      H._host_ptr(q), s.n, H._dt(tdt), float(S.EB), float(c.sf), s.mode, lo, hi, out)
    return [("code", rc, S.REFUSALS[kind])]


_IMPL = {"decompress": _decompress, "compress_nd": _compress_nd, "decompress_nd": _decompress_nd, "range": _range, "dct_blocks": _dct,
         "compress_batch": _batch, "decompress_batch": _batch, "deflate": _deflate, "inflate": _deflate, "epoch": _state}
_IMPL.update({k: _compress for k in ("compress", "compress_scaled", "compress_inplace", "compress_coef")})
_IMPL.update({k: _box for k in ("box", "boxes", "box_nd", "boxes_nd")})
_IMPL.update({k: _coarse for k in ("coarse", "coarse_nd")})
_IMPL.update({k: _coarse_box for k in ("coarse_box_nd", "coarse_boxes_nd")})
_IMPL.update({k: _summary for k in ("summary", "summary_ref", "summary_nd", "summary_nd_ref")})
_IMPL.update({k: _fixup for k in S.OPS if k.startswith("fixup")})
_IMPL.update({k: _mask for k in ("mask_build", "mask_build_nd", "compress_masked", "compress_masked_nd", "mask_apply")})
_IMPL.update({k: _rd for k in ("rd_probe", "rd_probe_nd", "compress_psnr", "compress_psnr_nd", "psnr_terms")})
_IMPL.update({k: _state for k in S.STATE_OPS})
_IMPL.update({k: _refusal for k in S.REFUSALS})
assert set(_IMPL) == set(S.KINDS) | {"epoch"}


# ---- E2: every (op, subject) as the first work call of a fresh context, once per module ---------------------------------------
_E2 = {}


def _e2(op):
    key = S.e2_key(*op)
    if key not in _E2:
        rec = {}
        r = Runner(record=rec, persistent=4 << 20, transient=16 << 20)
        try:
            r.run((op[0], op[1], {k: v for k, v in op[2].items() if k not in ("slot", "ctx")}), "fresh context")
        finally:
            r.close()
        _E2[key] = rec
    return _E2[key]
