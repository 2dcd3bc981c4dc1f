"""Batch items that share or alias buffers (include/dctz_hip.h, the comment above dctzhip_batch_citem).

Every item compresses its d_in as it was when the call was made, whatever its siblings do: several items may read one input
(a bound sweep over one array), an item may scale its own input in place (d_scaled == d_in, the reference's
dctz-comp-lib.c:193-216) while others read the same bytes, and the in-place division lands after every read of the call --
inside one launch sequence, across sequences of 1024 items, on the single-array path of the big items, on the redo of a
refused speculative item and across the two chains of a mixed batch.  Overlaps the call cannot honour (two in-place items on
one range, an output over any input or other output, a scaled copy partly over an input) are refused with DCTZHIP_E_ARG
before anything is launched.  The host-buffer batch dctz_compress_batch is byte for byte the loop of dctz_compress().

Every item is checked bit for bit against the oracle on a copy of its input taken before the call, and every buffer the
items live in is checked after it: in-place ranges hold the oracle's x / sf, everything else is as it was."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from tests.test_gpu_batch import _check_compress, _unsampled_element, spec_ctx  # noqa: F401  (spec_ctx: a fixture)

pytestmark = pytest.mark.gpu

MODES = [O.EC, O.QT]
DTYPES = [np.float64, np.float32]
N_SHORT = 4096 * 3 + 64 * 5 + 33          # several tiles and a short last block


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


@pytest.fixture()
def chain(ctx):
    """The chain of batch kernels (one-launch off) for one test."""
    ctx.set_one_launch(False)
    yield ctx
    ctx.set_one_launch(True)


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


class Pool:
    """Device buffers as byte allocations; items are (buffer, byte offset, n, dtype) views into them, so that several items
    can name the same or overlapping bytes."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def buf(self, nbytes):
        import torch
        b = torch.zeros(nbytes, dtype=torch.uint8, device=self.ctx.device)
        self.bufs.append(b)
        return len(self.bufs) - 1

    def put(self, bi, off, x):
        import torch
        raw = np.ascontiguousarray(x).view(np.uint8)
        self.bufs[bi][off:off + raw.size].copy_(torch.from_numpy(raw.copy()))

    def view(self, bi, off, n, dtype):
        es = np.dtype(dtype).itemsize
        assert off % 16 == 0 and off + n * es <= self.bufs[bi].numel()
        v = self.bufs[bi][off:off + n * es].view(_tdt(dtype))
        assert v.numel() == n
        return v

    def snapshot(self):
        return [b.cpu().numpy().copy() for b in self.bufs]

    def restore(self, snaps):
        import torch
        for b, s in zip(self.bufs, snaps):
            b.copy_(torch.from_numpy(s))


def _run_batch(ctx, pool, items, mode):
    """items: (buffer, byte offset, n, dtype, eb, in_place).  One compress_batch, every item against the oracle on its input
    as it was, the final contents of every buffer, then the same call again through `prepared=` on restored inputs."""
    import torch
    snaps = pool.snapshot()
    xs = [pool.view(bi, off, n, dt) for bi, off, n, dt, _, _ in items]
    host = [snaps[bi][off:off + n * np.dtype(dt).itemsize].view(dt).copy() for bi, off, n, dt, _, _ in items]
    ebs = [e for *_, e, _ in items]
    scaled = [x if ip else None for x, (*_, ip) in zip(xs, items)]
    outs, infos, prep = ctx.compress_batch(xs, ebs, mode, scaled=scaled)
    torch.cuda.synchronize()
    cs = [_check_compress(x, eb, mode, out, info) for x, eb, out, info in zip(host, ebs, outs, infos)]
    want = [s.copy() for s in snaps]
    for (bi, off, n, dt, _, ip), c in zip(items, cs):
        if ip:
            raw = np.ascontiguousarray(c.scaled).view(np.uint8)
            want[bi][off:off + raw.size] = raw

    def final_buffers():
        for i, (b, w) in enumerate(zip(pool.bufs, want)):
            assert np.array_equal(b.cpu().numpy(), w), f"buffer {i}: not the inputs as they were with x / sf over the in-place ranges"

    final_buffers()
    keep = [{k: v.clone() for k, v in o.items()} for o in outs]
    kinfo = [(i.sf, i.cnt, i.max_abs, i.min_abs, list(i.qtable[:])) for i in infos]
    pool.restore(snaps)
    outs2, infos2, _ = ctx.compress_batch(None, None, mode, prepared=prep)
    torch.cuda.synchronize()
    for j, (o, k, i, ki) in enumerate(zip(outs2, keep, infos2, kinfo)):
        assert (i.sf, i.cnt, i.max_abs, i.min_abs, list(i.qtable[:])) == ki, j
        for name in ("bin_index", "dc"):
            assert torch.equal(o[name], k[name]), (j, name)
        assert torch.equal(o["ac_exact"][:i.cnt], k["ac_exact"][:i.cnt]), j
    final_buffers()
    return outs, infos, cs


def _shared(ctx, n, dtype, positions, ebs, seed=0, scale=37.0):
    """One input under several bounds; the items at `positions` scale it in place."""
    pool = Pool(ctx)
    es = np.dtype(dtype).itemsize
    b = pool.buf(n * es)
    pool.put(b, 0, W.ragged(n, dtype, seed=seed, scale=scale))
    return pool, [(b, 0, n, dtype, eb, j in positions) for j, eb in enumerate(ebs)]


# ---- what the call already honoured: the in-place member of a bound sweep ----

@pytest.mark.parametrize("one", [False, True], ids=["chain", "one_launch"])
@pytest.mark.parametrize("where", [0, 2, 3], ids=["first", "middle", "last"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_bound_sweep_with_an_in_place_member(ctx, mode, dtype, where, one):
    ctx.set_one_launch(one)
    try:
        pool, items = _shared(ctx, N_SHORT, dtype, {where}, [1e-3, 1e-4, 1e-5, 1e-6])
        _run_batch(ctx, pool, items, mode)
    finally:
        ctx.set_one_launch(True)


# ---- case 1: the redo of a refused speculative item ----

@pytest.mark.parametrize("in_place_first", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_redo_of_a_refused_guess_reads_the_input_as_it_was(spec_ctx, dtype, in_place_first):
    """A spike between the sample's chunks of the shared input: the reader's guess is refused and the reader is compressed again
    on its own -- from the input as it was, not from what its in-place sibling made of it."""
    n = 1 << 20
    pool = Pool(spec_ctx)
    es = np.dtype(dtype).itemsize
    b, o = pool.buf(n * es), pool.buf(n * 8)
    x = W.ragged(n, dtype, seed=2, scale=37.0)
    x[_unsampled_element(dtype, 5)] = 4321.0
    pool.put(b, 0, x)
    pool.put(o, 0, W.ragged(n, np.float64, seed=3, scale=37.0))
    pair = [(b, 0, n, dtype, 1e-4, True), (b, 0, n, dtype, 1e-3, False)]
    items = (pair if in_place_first else pair[::-1]) + [(o, 0, n, np.float64, 1e-3, False)]
    _run_batch(spec_ctx, pool, items, O.EC)
    # the call: both items over the spiked input guessed and missed (the in-place one is planned as a reader, its division
    # deferred), the other array guessed right; the re-issue falls in the pause that follows a miss
    assert spec_ctx.counter(8) == 3 and spec_ctx.counter(9) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_guess_beside_an_in_place_sibling_with_one_launch(spec_ctx, dtype):
    spec_ctx.set_one_launch(True)
    n = 1 << 20
    pool = Pool(spec_ctx)
    b = pool.buf(n * np.dtype(dtype).itemsize)
    x = W.ragged(n, dtype, seed=2, scale=37.0)
    x[_unsampled_element(dtype, 5)] = 4321.0
    pool.put(b, 0, x)
    _run_batch(spec_ctx, pool, [(b, 0, n, dtype, 1e-3, False), (b, 0, n, dtype, 1e-4, True)], O.EC)


# ---- case 2: sequences split at 1024 items ----

def _across_sequences(ctx, mode, dtype):
    rng = np.random.default_rng(11)
    pool = Pool(ctx)
    es = np.dtype(dtype).itemsize
    b = pool.buf(N_SHORT * es)
    pool.put(b, 0, W.ragged(N_SHORT, dtype, seed=4, scale=420.0))
    items = [(b, 0, N_SHORT, dtype, 1e-3, True)]
    for i in range(1030):                                            # tiny fillers of the same element type
        n = int(rng.integers(1, 100))
        f = pool.buf(n * es)
        pool.put(f, 0, W.ragged(n, dtype, seed=100 + i, scale=5.0))
        items.append((f, 0, n, dtype, 1e-3, False))
    items.append((b, 0, N_SHORT, dtype, 1e-5, False))               # index 1031: the second sequence
    _run_batch(ctx, pool, items, mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_reader_in_a_later_sequence_than_the_in_place_item(chain, mode, dtype):
    _across_sequences(chain, mode, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reader_in_a_later_sequence_with_one_launch(ctx, dtype):
    _across_sequences(ctx, O.EC, dtype)


# ---- case 3: items for the single-array path ----

@pytest.mark.parametrize("in_place_first", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_big_items_that_share_an_input(chain, mode, in_place_first):
    n = (1 << 24) + 64 * 3 + 5
    pos = {0} if in_place_first else {1}
    pool, items = _shared(chain, n, np.float64, pos, [1e-3, 1e-5])
    _run_batch(chain, pool, items, mode)


# ---- case 5: the two chains of a mixed batch ----

def _fp32_over_fp64(ctx, mode):
    """An fp32 item scaled in place over bytes an fp64 item reads.  (Finite floats without zeros read as finite doubles.)"""
    rng = np.random.default_rng(5)
    n32 = 2 * N_SHORT
    x = (np.sin(np.arange(n32) * 0.01) * 3.0 + rng.normal(0, 0.01, n32)).astype(np.float32)
    x[np.abs(x) < 1e-3] = 1e-3
    pool = Pool(ctx)
    b = pool.buf(n32 * 4)
    pool.put(b, 0, x)
    o = pool.buf(5000 * 8)
    pool.put(o, 0, W.ragged(5000, np.float64, seed=6, scale=3.0))
    items = [(b, 0, N_SHORT, np.float64, 1e-3, False), (b, 0, n32, np.float32, 1e-4, True), (o, 0, 5000, np.float64, 1e-3, False)]
    _run_batch(ctx, pool, items, mode)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_in_place_fp32_over_an_fp64_reader(chain, mode):
    _fp32_over_fp64(chain, mode)


def test_mixed_batch_in_place_fp32_over_an_fp64_reader_with_one_launch(ctx):
    _fp32_over_fp64(ctx, O.EC)


# ---- a reader of a sub-range of an in-place buffer ----

@pytest.mark.parametrize("one", [False, True], ids=["chain", "one_launch"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_reader_of_a_sub_range_of_an_in_place_buffer(ctx, mode, dtype, one):
    ctx.set_one_launch(one)
    try:
        es = np.dtype(dtype).itemsize
        pool = Pool(ctx)
        b = pool.buf(N_SHORT * es)
        pool.put(b, 0, W.ragged(N_SHORT, dtype, seed=8, scale=37.0))
        skip = 16 * 129 // es                                         # 129 x 16 bytes in: not on a block boundary
        items = [(b, 16 * 129, 4096 + 64 * 2 + 9, dtype, 1e-4, False), (b, 0, N_SHORT, dtype, 1e-3, True),
                 (b, 16 * 129 + es * 4096, N_SHORT - skip - 4096, dtype, 1e-5, False)]
        _run_batch(ctx, pool, items, mode)
    finally:
        ctx.set_one_launch(True)


# ---- the one-launch give-up ----

@pytest.mark.parametrize("mode", MODES)
def test_one_launch_gives_up_on_a_batch_with_an_in_place_member(mode):
    """dctzhip_debug_knob(ctx, 0, 1): the one-launch kernel gives up and the arrays it held are run through the chain."""
    import dctz_amd
    c = dctz_amd.Context(0)
    try:
        pool, items = _shared(c, N_SHORT, np.float64, {1}, [1e-3, 1e-4, 1e-5])
        o = pool.buf(5000 * 4)
        pool.put(o, 0, W.ragged(5000, np.float32, seed=9, scale=3.0))
        items.append((o, 0, 5000, np.float32, 1e-3, False))
        c.knob(0, 1)
        _run_batch(c, pool, items, mode)
        assert c.counter(1) >= 1                                      # (ONE_GAVE_UP: the launch did give up)
        c.knob(0, 0)
    finally:
        c.close()


# ---- overlaps the call refuses ----

def _refused(fn, ctx, bufs):
    import dctz_amd
    before = [b.cpu().numpy().copy() for b in bufs]
    with pytest.raises(dctz_amd.hip.DctzHipError) as e:
        fn()
    import torch
    torch.cuda.synchronize()
    assert f"({dctz_amd.hip.E_ARG})" in str(e.value), str(e.value)
    for i, (b, w) in enumerate(zip(bufs, before)):
        assert np.array_equal(b.cpu().numpy(), w), f"buffer {i} was written by a refused call"


class Arena:
    """Every buffer of one call as a view of ONE allocation, filled with a sentinel, with room behind every view for what a
    kernel could write there (a refused call writes nothing; an accepted one stays in bounds)."""

    def __init__(self, ctx, nbytes):
        import torch
        self.a = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=ctx.device)

    def v(self, off, n, tdt):
        import torch
        es = torch.empty(0, dtype=tdt).element_size()
        assert off % 16 == 0 and off + n * es <= self.a.numel()
        t = self.a[off:off + n * es].view(tdt)
        assert t.numel() == n
        return t

    def outs(self, off_bin, off_dc, off_ac, n):
        import torch
        return {"bin_index": self.v(off_bin, n, torch.uint8), "dc": self.v(off_dc, (n + 63) // 64, torch.float32),
                "ac_exact": self.v(off_ac, n, torch.float32)}


def _arena_input(ar, off, x):
    import torch
    t = ar.v(off, x.size, _tdt(x.dtype))
    t.copy_(torch.from_numpy(x))
    return t


N_ARG = 4096 + 64 * 3 + 17
MB = 1 << 20


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["two_in_place_same", "two_in_place_overlap", "scaled_partly_over_own_input",
                                  "scaled_partly_over_other_input", "scaled_onto_other_input", "bin_inside_other_input",
                                  "outputs_shared", "dc_over_ac"])
def test_batch_overlaps_are_refused(ctx, dtype, case):
    import torch
    es = np.dtype(dtype).itemsize
    n = N_ARG
    ar = Arena(ctx, 16 * MB)
    x0 = _arena_input(ar, 0, W.ragged(n, dtype, seed=1, scale=37.0))
    x1 = _arena_input(ar, 2 * MB, W.ragged(n, dtype, seed=2, scale=5.0))
    outs = [ar.outs(4 * MB, 5 * MB, 6 * MB, n), ar.outs(8 * MB, 9 * MB, 10 * MB, n)]
    xs, scaled = [x0, x1], [None, None]
    if case == "two_in_place_same":
        xs, scaled = [x0, x0], [x0, x0]
    elif case == "two_in_place_overlap":
        xs[1] = ar.v(16 * 64, n, _tdt(dtype)); scaled = [x0, xs[1]]
    elif case == "scaled_partly_over_own_input":
        scaled[0] = ar.v(16, n, _tdt(dtype))
    elif case == "scaled_partly_over_other_input":
        scaled[0] = ar.v(2 * MB + 16 * 8, n, _tdt(dtype))
    elif case == "scaled_onto_other_input":
        scaled[0] = x1
    elif case == "bin_inside_other_input":
        outs[0]["bin_index"] = ar.v(2 * MB + 16 * 4, n, torch.uint8)
    elif case == "outputs_shared":
        outs[1] = ar.outs(4 * MB, 9 * MB, 10 * MB, n)
    elif case == "dc_over_ac":
        outs[1]["dc"] = ar.v(6 * MB + es * 64, (n + 63) // 64, torch.float32)
    _refused(lambda: ctx.compress_batch(xs, [1e-3, 1e-4], O.EC, outs=outs, scaled=scaled), ctx, [ar.a])


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_compress_with_a_scaled_copy_partly_over_its_input_is_refused(ctx, dtype):
    ar = Arena(ctx, 8 * MB)
    x = _arena_input(ar, 0, W.ragged(N_ARG, dtype, seed=3, scale=37.0))
    out = ar.outs(2 * MB, 3 * MB, 4 * MB, N_ARG)
    _refused(lambda: ctx.compress(x, 1e-3, O.EC, out=out, scaled=ar.v(16, N_ARG, _tdt(dtype))), ctx, [ar.a])
    _refused(lambda: ctx.compress(x, 1e-3, O.EC, out=ar.outs(16 * 4, 3 * MB, 4 * MB, N_ARG)), ctx, [ar.a])


class _Off:
    """A stream buffer as the wrapper reads it (data_ptr), `nbytes` past the tensor's start."""

    def __init__(self, t, nbytes):
        self._p = t.data_ptr() + nbytes

    def data_ptr(self):
        return self._p


def _streams_in_arena(ctx, dtype, mode):
    """A compressed array whose streams live in an arena at 0 / 1 MiB / 2 MiB, and its oracle record."""
    import torch
    x = np.random.default_rng(5).random(N_ARG).astype(dtype)      # noise: plenty of exact coefficients
    ar = Arena(ctx, 16 * MB)
    out = ar.outs(0, 1 * MB, 2 * MB, N_ARG)
    _, info = ctx.compress(torch.from_numpy(x).to(ctx.device), 1e-3, mode, out=out)
    torch.cuda.synchronize()
    c = _check_compress(x, 1e-3, mode, out, info)
    assert c.cnt > 0
    return ar, out, c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_output_over_its_streams_is_refused(ctx, dtype, mode):
    ar, out, c = _streams_in_arena(ctx, dtype, mode)
    tdt = _tdt(dtype)
    for at in (0, 1 * MB, 2 * MB - 16 * 3):                          # over bin_index, DC, AC_exact
        dst = ar.v(at, N_ARG, tdt)
        _refused(lambda: ctx.decompress(out, c.cnt, N_ARG, tdt, 1e-3, c.sf, mode, qtable=c.qtable, dst=dst), ctx, [ar.a])
        good = ar.v(8 * MB, N_ARG, tdt)
        _refused(lambda: ctx.decompress_batch([out, out], [c.cnt] * 2, [N_ARG] * 2, [tdt] * 2, 1e-3, [c.sf] * 2, mode,
                                              qtables=[c.qtable] * 2, dsts=[good, dst]), ctx, [ar.a])
    # DC or AC_exact 2 bytes off a 4-byte boundary (include/dctz_hip.h: DC, AC_exact: 4-byte aligned)
    good = ar.v(8 * MB, N_ARG, tdt)
    for key in ("dc", "ac_exact"):
        off = dict(out, **{key: _Off(out[key], 2)})
        _refused(lambda: ctx.decompress(off, c.cnt, N_ARG, tdt, 1e-3, c.sf, mode, qtable=c.qtable, dst=good), ctx, [ar.a])
        _refused(lambda: ctx.decompress_batch([out, off], [c.cnt] * 2, [N_ARG] * 2, [tdt] * 2, 1e-3, [c.sf] * 2, mode,
                                              qtables=[c.qtable] * 2, dsts=[good, ar.v(9 * MB, N_ARG, tdt)]), ctx, [ar.a])
    # two decode outputs over each other
    d0, d1 = ar.v(8 * MB, N_ARG, tdt), ar.v(8 * MB + 16 * 5, N_ARG, tdt)
    _refused(lambda: ctx.decompress_batch([out, out], [c.cnt] * 2, [N_ARG] * 2, [tdt] * 2, 1e-3, [c.sf] * 2, mode,
                                          qtables=[c.qtable] * 2, dsts=[d0, d1]), ctx, [ar.a])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_batch_items_may_share_their_streams(ctx, dtype, mode):
    import torch
    ar, out, c = _streams_in_arena(ctx, dtype, mode)
    tdt = _tdt(dtype)
    k = 5
    dsts = [ar.v(8 * MB + i * MB, N_ARG, tdt) for i in range(k)]
    _, status, _ = ctx.decompress_batch([out] * k, [c.cnt] * k, [N_ARG] * k, [tdt] * k, 1e-3, [c.sf] * k, mode,
                                        qtables=[c.qtable] * k, dsts=dsts)
    torch.cuda.synchronize()
    assert status == [0] * k
    want = O.decompress(c, O.FAST)
    for d in dsts:
        assert np.array_equal(d.cpu().numpy().view(np.uint8), want.view(np.uint8))


# ---- case 6: the host-buffer batch ----

@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_host_batch_with_shared_buffers_is_the_looped_calls(mode):
    """dctz_compress_batch with one t_var twice, and with two t_vars over one host buffer under different bounds: the
    containers, outSizes and the final arrays of the loop of dctz_compress() calls in index order (the second call over a
    buffer reads what the first one's in-place scaling left there), the same twice over."""
    from tests.test_libdctz_gpu import TVar, _lib, _tvar
    lib = _lib(mode)
    PT = C.POINTER(TVar)
    lib.dctz_compress_batch.restype = C.c_int
    lib.dctz_compress_batch.argtypes = [C.c_int, C.POINTER(PT), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(PT), C.POINTER(C.c_double)]
    a = W.c5_fp64(W.MSST19_LENGTHS[0], 3)
    b = W.ragged(64 * 200 + 21, np.float32, scale=5.0)
    c = W.c5_fp64(W.MSST19_LENGTHS[1], 4)
    ebs = [1e-3, 1e-4, 1e-3, 1e-5, 1e-4]

    def layout():
        """(arrays, per item: (array index, use the same t_var as item j or None))"""
        arrs = [a.copy(), b.copy(), c.copy()]
        return arrs, [(0, None), (1, None), (0, 0), (2, None), (2, None)]   # item 2: item 0's t_var; items 3, 4: one buffer

    def looped():
        arrs, spec = layout()
        vars_ = []
        for ai, same in spec:
            vars_.append(vars_[same] if same is not None else _tvar(arrs[ai]))
        zs = [np.zeros(arrs[ai].nbytes + 4096, np.uint8) for ai, _ in spec]
        sizes = []
        for v, z, eb, (ai, _) in zip(vars_, zs, ebs, spec):
            var_z = TVar()
            var_z.datatype = v.datatype
            var_z.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
            out = C.c_size_t(0)
            assert lib.dctz_compress(C.byref(v), arrs[ai].size, C.byref(out), C.byref(var_z), eb) == 1
            sizes.append(out.value)
        return arrs, [z[:s].copy() for z, s in zip(zs, sizes)], sizes

    def batched():
        arrs, spec = layout()
        vars_ = []
        for ai, same in spec:
            vars_.append(vars_[same] if same is not None else _tvar(arrs[ai]))
        zs = [np.zeros(arrs[ai].nbytes + 4096, np.uint8) for ai, _ in spec]
        vars_z = []
        for v, z in zip(vars_, zs):
            t = TVar()
            t.datatype = v.datatype
            t.buf.d = z.ctypes.data_as(C.POINTER(C.c_double))
            vars_z.append(t)
        k = len(spec)
        pv = (PT * k)(*[C.pointer(v) for v in vars_])
        pz = (PT * k)(*[C.pointer(v) for v in vars_z])
        ns = (C.c_int * k)(*[arrs[ai].size for ai, _ in spec])
        outs = (C.c_size_t * k)()
        assert lib.dctz_compress_batch(k, pv, ns, outs, pz, (C.c_double * k)(*ebs)) == 1
        return arrs, [z[:outs[i]].copy() for i, z in enumerate(zs)], list(outs)

    la, lz, ls = looped()
    for _ in range(2):
        ba, bz, bs = batched()
        assert bs == ls
        for i, (p, q) in enumerate(zip(bz, lz)):
            assert p.tobytes() == q.tobytes(), f"container {i}"
        for i, (p, q) in enumerate(zip(ba, la)):
            assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), f"array {i}"
