"""A list of boxes of one array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one call (include/dctz_hip.h:
dctzhip_decompress_boxes_nd).

Every output against the slice of the full dctzhip_decompress_nd and against dctzhip_decompress_box_nd for the same box, bit
for bit, and against the CPU oracle's decompress_nd; boxes that repeat, nest and share a stream tile; the work list follows
the hit stream tiles (dctzhip_debug_counter 13 against a count from a boolean mask over the block grid); the grid-stride
loop over the list; locality (everything outside the union of the hit tiles poisoned); output bounds (guards between and
around the outputs of one arena); the refusals, each followed by a good list call on the same context; the index check; a
NaN block.

The workloads, shapes, boxes and the poisoning are those of the single-box test (tests/test_gpu_ndbox_decode.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import nonfinite as NF
from tests import test_gpu_ndbox_decode as NB
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

BIG, GAPS, RAGGED3 = NB.BIG, NB.GAPS, NB.RAGGED3


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _list(ctx, data, shape, boxes, mode, out=None, idx=None, cnt=None, dsts=None):
    o, info, full, ix, eb, q, tdt = data
    return ctx.decompress_boxes_nd(out or o, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, boxes, ix if idx is None else idx,
                                   mode, qtable=q, dsts=dsts)


def _hits(shape, lo, hi):
    return int(NB._hit_tiles(shape, lo, hi)[0].sum())


def _candidates(shape, lo, hi):
    _, t0, t1 = NB._hit_tiles(shape, lo, hi)
    return t1 - t0


def _about_50(shape, seed):
    fixed = len(NB._boxes(shape, seed, k=0))
    return NB._boxes(shape, seed, k=max(8, 50 - fixed))


def _check_all(rs, full, shape, boxes):
    assert len(rs) == len(boxes)
    for r, (lo, hi) in zip(rs, boxes):
        assert tuple(r.shape) == tuple(h - l for l, h in zip(lo, hi))
        assert NB._same_dev(r, NB._slice(full, shape, lo, hi)), (lo, hi)


def _kernel_name(dtype, mode, shape):
    return f"k_decompress_mbox_nd<{'double' if dtype == np.float64 else 'float'}, {mode}, {len(shape) - 1}>"


@pytest.mark.parametrize("case", NB.CASES, ids=NB._id)
def test_every_output_is_the_slice_and_the_single_call(ctx, case):
    """Parity, and the list follows the hits: counter 13 (items listed) is the number of stream tiles with a block that
    intersects box i, summed over the boxes, from a boolean mask; it stays within the host's bound (counter 15)."""
    shape, kind, dtype, mode = case
    data = NB._case(ctx, shape, kind, dtype, mode)
    full = data[2]
    boxes = _about_50(shape, seed=11)
    rs = _list(ctx, data, shape, boxes, mode)
    items, bound = ctx.counter(13), ctx.counter(15)
    assert ctx.last_kernel(1) == _kernel_name(dtype, mode, shape)
    _check_all(rs, full, shape, boxes)
    assert items == sum(_hits(shape, lo, hi) for lo, hi in boxes)
    assert items <= bound
    for r, (lo, hi) in zip(rs, boxes):
        assert NB._same_dev(r, NB._box(ctx, data, shape, lo, hi, mode)), (lo, hi)
    # k = 1
    lo, hi = NB._odd_box(shape)
    (r,) = _list(ctx, data, shape, [(lo, hi)], mode)
    assert NB._same_dev(r, NB._box(ctx, data, shape, lo, hi, mode))
    (r,) = _list(ctx, data, shape, [(lo, hi)], mode)
    assert ctx.counter(13) == _hits(shape, lo, hi) and ctx.counter(13) <= ctx.counter(15)
    assert ctx.last_kernel(1) == _kernel_name(dtype, mode, shape)


@pytest.mark.parametrize("case", NB.ORACLE, ids=lambda c: NB._id((c[0], "ragged", c[1], c[2])))
def test_every_output_is_the_slice_of_the_oracle(ctx, case):
    import oracle.oracle as O
    shape, dtype, mode = case
    data = NB._case(ctx, shape, "ragged", dtype, mode)
    x = NB._input(shape, "ragged", dtype)
    ref = O.decompress_nd(O.compress_nd(x, NB.EBS["ragged"], O.QT if mode == H.QT else O.EC), shape)
    u = np.uint64 if dtype == np.float64 else np.uint32
    boxes = NB._boxes(shape, seed=11, k=10)
    for r, (lo, hi) in zip(_list(ctx, data, shape, boxes, mode), boxes):
        r = r.cpu().numpy()
        want = np.ascontiguousarray(ref[tuple(slice(l, h) for l, h in zip(lo, hi))])
        assert r.shape == want.shape and np.array_equal(r.view(u), want.view(u)), (lo, hi)


SHARED = {(16, 16, 32): (((0, 0, 0), (4, 4, 16)), ((0, 0, 16), (4, 4, 32))), (45, 77): (((0, 0), (8, 40)), ((0, 40), (8, 77)))}


@pytest.mark.parametrize("case", [c for c in NB.CASES if c[0] in SHARED and c[1] == "ragged"], ids=NB._id)
def test_boxes_may_repeat_nest_and_share_a_tile(ctx, case):
    shape, kind, dtype, mode = case
    data = NB._case(ctx, shape, kind, dtype, mode)
    odd = NB._odd_box(shape)
    outer = (tuple(d // 5 for d in shape), tuple(d - d // 5 for d in shape))
    inner = (tuple(l + 1 for l in outer[0]), tuple(max(l + 2, h - 1) for l, h in zip(outer[0], outer[1])))
    a, b = SHARED[shape]                               # two boxes in the first stream tile without a common element
    assert any(ah <= bl for ah, bl in zip(a[1], b[0]))
    assert _hits(shape, *a) == 1 and _hits(shape, *b) == 1
    assert NB._hit_tiles(shape, *a)[1] == NB._hit_tiles(shape, *b)[1] == 0
    boxes = [odd, odd, odd, outer, inner, a, b]
    rs = _list(ctx, data, shape, boxes, mode)
    _check_all(rs, data[2], shape, boxes)
    assert ctx.counter(13) == sum(_hits(shape, lo, hi) for lo, hi in boxes)       # duplicates counted


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_thin_slabs_list_fewer_items_than_candidates(ctx, dtype):
    """(12, 64, 256): 3 x 16 x 64 blocks, a stream tile is one (z, y) block row, 48 tiles in all.  The one-thick slabs along
    axes 0 and 2 hit every one of their candidates (16 and 48); the slab along axis 1 hits one tile per block plane, 3 of
    33 candidates.  Every list but {slab 0, slab 2} lists exactly its hits and strictly fewer items than candidates."""
    shape, mode = GAPS, H.EC
    data = NB._case(ctx, shape, "ragged", dtype, mode)
    slabs = []
    for a in range(3):
        at = shape[a] // 3
        slabs.append((tuple(at if i == a else 0 for i in range(3)), tuple(at + 1 if i == a else shape[i] for i in range(3))))
    assert NB._nblk(shape) // NB.TILE_BLKS == 48
    assert [(_hits(shape, *s), _candidates(shape, *s)) for s in slabs] == [(16, 16), (3, 33), (48, 48)]
    for boxes in ([slabs[0], slabs[2]], slabs, NB.LOCAL_BOXES[GAPS]) + tuple([bx] for bx in NB.LOCAL_BOXES[GAPS]):
        rs = _list(ctx, data, shape, boxes, mode)
        _check_all(rs, data[2], shape, boxes)
        items, cand = ctx.counter(13), sum(_candidates(shape, lo, hi) for lo, hi in boxes)
        assert items == sum(_hits(shape, lo, hi) for lo, hi in boxes)
        if boxes == [slabs[0], slabs[2]]:
            assert items == cand                       # nothing to skip in these two
        else:
            assert items < cand, (boxes, items, cand)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_workgroups_take_several_items(ctx, dtype):
    shape = BIG
    data = NB._case(ctx, shape, "ragged", dtype, H.EC)
    full_box = ((0, 0, 0), shape)
    rs = _list(ctx, data, shape, [full_box] * 3, H.EC)
    assert ctx.counter(13) == 3 * (NB._nblk(shape) // NB.TILE_BLKS) == 7680
    assert ctx.counter(14) < ctx.counter(13)
    for r in rs:
        assert NB._same_dev(r, data[2])


@pytest.mark.parametrize("case", NB.LOCAL, ids=NB._id)
def test_list_reads_only_the_union_of_the_hit_tiles(ctx, case):
    """Everything outside the union of the hit tiles of LOCAL_BOXES[shape] is poisoned.  On (16, 520) and (16, 16, 32) -- 3
    and 2 stream tiles -- the three boxes together hit every tile (from the mask), so nothing would be poisoned there:
    on these two the sub-lists that leave a tile without a hit are run as well, and at least one must exist."""
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = NB._case(ctx, shape, kind, dtype, mode)
    boxes = NB.LOCAL_BOXES[shape]

    def union(bx):
        hit = np.zeros_like(NB._hit_tiles(shape, *bx[0])[0])
        for lo, hi in bx:
            hit |= NB._hit_tiles(shape, lo, hi)[0]
        return hit

    lists = [boxes]
    if union(boxes).all():
        subs = [list(s) for r in range(len(boxes) - 1, 0, -1) for s in itertools.combinations(boxes, r)]
        lists += [s for s in subs if not union(s).all()]
    assert not union(lists[-1]).all(), "every tile is hit by some box: nothing is poisoned"
    for bx in lists:
        hit = union(bx)
        t = np.flatnonzero(hit)
        if shape in (GAPS, BIG):                       # tiles BETWEEN hit ones that no box of the list hits
            assert (~hit[t[0]:t[-1] + 1]).sum() >= 2
        pout, pix = NB._poisoned(out, idx, NB._nblk(shape), hit, seed=3)
        rs = _list(ctx, data, shape, bx, mode, out=pout, idx=pix)
        _check_all(rs, full, shape, bx)


@pytest.mark.parametrize("case", NB.GUARDED, ids=NB._id)
def test_list_writes_only_its_outputs(ctx, case):
    """The outputs carved out of one arena, 64-byte guards between and around them (and the bytes up to the next 16-byte
    boundary behind an output): every byte that belongs to no output keeps its pattern."""
    import torch
    shape, kind, dtype, mode = case
    data = NB._case(ctx, shape, kind, dtype, mode)
    tdt = data[6]
    es = 8 if dtype == np.float64 else 4
    boxes = NB._corners(shape) + [NB._odd_box(shape), NB._aligned(shape), ((0,) * len(shape), tuple(shape)), NB._odd_box(shape)]
    at, spans = 64, []
    for lo, hi in boxes:
        nb = int(np.prod([h - l for l, h in zip(lo, hi)])) * es
        spans.append((at, nb))
        at = (at + nb + 15) // 16 * 16 + 64
    arena = torch.full((at,), 0x5A, dtype=torch.uint8, device=ctx.device)
    assert arena.data_ptr() % 16 == 0
    dsts = [arena[a:a + nb].view(tdt) for a, nb in spans]
    rs = _list(ctx, data, shape, boxes, mode, dsts=dsts)
    _check_all(rs, data[2], shape, boxes)
    mine = torch.zeros(at, dtype=torch.bool, device=ctx.device)
    for a, nb in spans:
        mine[a:a + nb] = True
    assert bool((arena[~mine] == 0x5A).all())
    assert int((~mine).sum()) >= 64 * (len(boxes) + 1)


def _raw(ctx, out, cnt, tdt, eb, sf, dims, items, idx_ptr, mode, q, k=None, null=False, nd=None, bin_ptr=None):
    """items: (lo, hi, output pointer) per box; k (or None: their number) is what the call is told."""
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = (H.BoxItem * max(len(items), 1))()
    for it, (lo, hi, ptr) in zip(arr, items):
        for i, (l, h) in enumerate(zip(lo, hi)):
            it.lo[i], it.hi[i] = l, h
        it.d_out = ptr
    return ctx.lib.dctzhip_decompress_boxes_nd(ctx.h, out["bin_index"].data_ptr() if bin_ptr is None else bin_ptr, out["dc"].data_ptr(),
                                               out["ac_exact"].data_ptr(), int(cnt), idx_ptr, qp, len(dims) if nd is None else nd,
                                               (C.c_size_t * len(dims))(*dims), H._dt(tdt), float(eb), float(sf), mode,
                                               len(items) if k is None else k, None if null else C.cast(arr, C.c_void_p))


# four boxes of (12, 64, 256); box 0 has 25 elements (24 of them a multiple of 16 bytes in either element type)
REF_BOXES = [((0, 0, 0), (1, 5, 5)), ((1, 3, 100), (3, 5, 200)), ((0, 63, 0), (12, 64, 256)), ((2, 7, 9), (3, 20, 60))]


@pytest.mark.parametrize("case", [c for c in NB.CASES if c[0] == GAPS], ids=NB._id)
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = NB._case(ctx, shape, kind, dtype, mode)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    es = 8 if dtype == np.float64 else 4
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    sizes = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in REF_BOXES]
    starts = [0, 1024, 2048, 8192]                      # elements of one arena, 16-byte aligned
    assert all(s + z <= e for s, z, e in zip(starts, sizes, starts[1:] + [16384]))
    arena = torch.empty(16384, dtype=tdt, device=ctx.device)
    NB._ivw(arena).fill_(0x5A5A5A5A)
    sentinel = arena.clone()
    ptr = lambda i: arena.data_ptr() + starts[i] * es
    good = [(lo, hi, ptr(i)) for i, (lo, hi) in enumerate(REF_BOXES)]

    def swap(i, lo=None, hi=None, p=None):
        v = list(good)
        v[i] = (v[i][0] if lo is None else lo, v[i][1] if hi is None else hi, v[i][2] if p is None else p)
        return v

    def call(items=good, dims=shape, qq=q, **kw):
        return _raw(ctx, cp, info.cnt, tdt, eb, info.sf, dims, items, idx.data_ptr(), mode, qq, **kw)

    def untouched():
        assert NB._same_dev(arena, sentinel)
        for k in out:
            bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
            assert torch.equal(bits(cp[k]), bits(out[k])), k

    def good_call():
        assert call() == H.OK
        for i, (lo, hi) in enumerate(REF_BOXES):
            r = arena[starts[i]:starts[i] + sizes[i]].view([h - l for l, h in zip(lo, hi)])
            assert NB._same_dev(r, NB._slice(full, shape, lo, hi)), (lo, hi)
        arena.copy_(sentinel)

    good_call()
    many = [good[0]] * (H.BOXES_MAX + 1)
    # bin ids that box 1 reads: its first candidate stream tile
    t0_1 = NB._hit_tiles(shape, *REF_BOXES[1])[1]
    bin_at = cp["bin_index"].data_ptr() + 4096 * t0_1
    refused = [
        dict(k=0), dict(items=many), dict(null=True),
        dict(items=swap(2, hi=(12, 65, 256))),                                         # box 2 of 4: hi > dims
        dict(items=swap(1, p=ptr(1) + es)),                                            # box 1: misaligned output
        dict(items=swap(3, p=ptr(0) + (sizes[0] - 1) * es)),                           # outputs of boxes 0 and 3: one element in common
        dict(items=swap(1, p=bin_at)),                                                 # an output over bin ids a box reads
        dict(nd=1, dims=shape[:1]), dict(nd=4, dims=tuple(shape) + (1,)),              # ndims must be 2 or 3
    ]
    if mode == H.QT:
        refused.append(dict(qq=None))                                                  # QT without its table
    assert (ptr(0) + (sizes[0] - 1) * es) % 16 == 0 and len(many) == 4097
    for kw in refused:
        assert call(**kw) == H.E_ARG, kw
        untouched()
        good_call()
    assert call(items=swap(2, hi=(12, 65, 256))) == H.E_ARG                            # the message names the box
    assert "box 2" in ctx.lib.dctzhip_last_error(ctx.h).decode()
    good_call()


@pytest.mark.parametrize("case", [c for c in NB.CASES if c[0] == GAPS], ids=NB._id)
def test_index_check_covers_the_hit_tiles_of_every_box(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = NB._case(ctx, shape, kind, dtype, mode)
    boxes = list(REF_BOXES)
    hits = [NB._hit_tiles(shape, lo, hi)[0] for lo, hi in boxes]
    others = hits[0] | hits[1] | hits[3]
    own = np.flatnonzero(hits[2] & ~others & ~np.roll(others, 1))                       # neither idx[t] nor idx[t + 1] of another box's tile
    own = [int(t) for t in own if not others[t + 1:t + 2].any()]
    assert own

    def good_call():
        _check_all(_list(ctx, data, shape, boxes, mode), full, shape, boxes)

    t = own[-1]
    ix = idx.clone()
    ix[t + 1] += 1                                     # tile t of box 2 alone: its flags no longer number idx[t + 1] - idx[t]
    with pytest.raises(H.DctzHipError):
        _list(ctx, data, shape, boxes, mode, idx=ix)
    rc = _raw(ctx, out, info.cnt, tdt, eb, info.sf, shape,
              [(lo, hi, r.data_ptr()) for (lo, hi), r in zip(boxes, _list(ctx, data, shape, boxes, mode))], ix.data_ptr(), mode,
              None if q is None else np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32))
    assert rc == H.E_ARG
    good_call()
    # ac_count one short of what the last hit tile of the list needs
    last = int(np.flatnonzero(hits[0] | hits[1] | hits[2] | hits[3])[-1])
    need = int(idx[last + 1])
    assert need > 0
    with pytest.raises(H.DctzHipError):
        _list(ctx, data, shape, boxes, mode, cnt=need - 1)
    good_call()
    _check_all(_list(ctx, data, shape, boxes, mode, cnt=need), full, shape, boxes)


@pytest.mark.parametrize("shape", [(45, 77), RAGGED3], ids=["45x77", "13x22x35"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_boxes_around_a_nan_block(ctx, shape, dtype, mode):
    """A NaN in one block: two boxes that straddle the block and one that avoids it; NaN exactly where the full decode has
    NaN, the same bits everywhere else (tests/nonfinite.py's rule)."""
    import torch
    x = NB._input(shape, "ragged", dtype)
    at = tuple(d // 2 for d in shape)
    x[at] = np.nan
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out, info = ctx.compress_nd(torch.from_numpy(x).to(ctx.device), 1e-3, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress_nd(out, info.cnt, shape, tdt, 1e-3, info.sf, mode, qtable=q)
    idx, _ = ctx.ac_index(out, 64 * NB._nblk(shape))
    e = NB.EDGE[len(shape)]
    boxes = [(tuple(max(0, a - e - 1) for a in at), tuple(min(d, a + e + 2) for a, d in zip(at, shape))),
             (tuple(max(0, a - 1) for a in at), tuple(shape)),
             ((0,) * len(shape), tuple(a // e * e for a in at))]                         # ends in front of the NaN's block on every axis
    rs = ctx.decompress_boxes_nd(out, info.cnt, shape, tdt, 1e-3, info.sf, boxes, idx, mode, qtable=q)
    for i, (r, (lo, hi)) in enumerate(zip(rs, boxes)):
        want = NB._slice(full, shape, lo, hi).cpu().numpy()
        assert np.isnan(want).any() == (i < 2) and not np.isnan(want).all()
        assert NF.same_with_nans(r.cpu().numpy(), want), NF.describe_mismatch(r.cpu().numpy(), want)
