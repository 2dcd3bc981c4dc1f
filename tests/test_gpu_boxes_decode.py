"""A list of boxes of one array in one call (include/dctz_hip.h: dctzhip_decompress_boxes).

Every output against the slice of a full decode and against dctzhip_decompress_box for the same box, bit for bit; boxes that
overlap, nest and repeat; the work list follows the hit tiles (dctzhip_debug_counter 13 against a count from a boolean mask);
the grid-stride loop over the list; locality (everything outside the union of the hit tiles poisoned); output bounds (guards
between and around the outputs of one arena); the short last block; the refusals, each followed by a good list call on the
same context; the index check; a NaN-poisoned tile.

The workloads, shapes, boxes and the poisoning are those of the single-box test, from tests/box_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import nonfinite as NF
from tests import box_cases as B
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

TILE = B.TILE
BIG, GAPS = B.BIG, B.GAPS
SHAPES = [(5, 7, 9), (33, 65, 67), (130, 1000), (6, 10, 12, 50), (64 * 777 + 45,), GAPS]
WORKLOADS = [(s, "ragged") for s in SHAPES] + [((33, 65, 67), "dense"), ((33, 65, 67), "none")]
CASES = [(s, kind, dt, mode) for s, kind in WORKLOADS for dt in (np.float64, np.float32) for mode in (H.EC, H.QT)]
CASES += [(BIG, "ragged", dt, H.EC) for dt in (np.float64, np.float32)]


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _list(ctx, data, shape, boxes, mode, out=None, idx=None, cnt=None, dsts=None):
    o, info, full, ix, eb, q, tdt = data
    return ctx.decompress_boxes(out or o, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, boxes, ix if idx is None else idx,
                                mode, qtable=q, dsts=dsts)


def _hits(shape, lo, hi):
    return int(B._hit_tiles(shape, lo, hi)[0].sum())


def _candidates(shape, lo, hi):
    _, t0, t1 = B._hit_tiles(shape, lo, hi)
    return t1 - t0


def _about_50(shape, seed):
    fixed = len(B._boxes(shape, seed, k=0))
    return B._boxes(shape, seed, k=max(8, 50 - fixed))


def _check_all(rs, full, shape, boxes):
    assert len(rs) == len(boxes)
    for r, (lo, hi) in zip(rs, boxes):
        assert tuple(r.shape) == tuple(h - l for l, h in zip(lo, hi))
        assert B._same_dev(r, B._slice(full, shape, lo, hi)), (lo, hi)


@pytest.mark.parametrize("case", CASES, ids=B._id)
def test_every_output_is_the_slice_and_the_single_call(ctx, case):
    """Parity, and the list follows the hits: counter 13 (items listed) is the number of tiles with an element in box i,
    summed over the boxes, from a boolean mask; it stays within the host's bound (counter 15)."""
    shape, kind, dtype, mode = case
    data = B._case(ctx, shape, kind, dtype, mode)
    full = data[2]
    boxes = _about_50(shape, seed=11)
    rs = _list(ctx, data, shape, boxes, mode)
    items, bound = ctx.counter(13), ctx.counter(15)
    assert ctx.last_kernel(1) == f"k_decompress_mbox<{'double' if dtype == np.float64 else 'float'}, {mode}>"
    _check_all(rs, full, shape, boxes)
    assert items == sum(_hits(shape, lo, hi) for lo, hi in boxes)
    assert items <= bound
    for r, (lo, hi) in zip(rs, boxes):
        assert B._same_dev(r, B._box(ctx, data, shape, lo, hi, mode)), (lo, hi)
    # k = 1
    lo, hi = B._odd_box(shape)
    (r,) = _list(ctx, data, shape, [(lo, hi)], mode)
    assert B._same_dev(r, B._box(ctx, data, shape, lo, hi, mode))
    assert ctx.counter(13) == _hits(shape, lo, hi)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((33, 65, 67), GAPS) and c[1] == "ragged"], ids=B._id)
def test_boxes_may_repeat_nest_and_share_a_tile(ctx, case):
    shape, kind, dtype, mode = case
    data = B._case(ctx, shape, kind, dtype, mode)
    odd = B._odd_box(shape)
    outer = (tuple(d // 5 for d in shape), tuple(d - d // 5 for d in shape))
    inner = (tuple(l + 1 for l in outer[0]), tuple(max(l + 2, h - 1) for l, h in zip(outer[0], outer[1])))
    # two boxes in the first tile (the first rows of plane 0) without a common element
    a = ((0, 0, 0), (1, 1, shape[2] // 2))
    b = ((0, 0, shape[2] // 2), (1, 1, shape[2]))
    assert shape[2] <= TILE
    boxes = [odd, odd, odd, outer, inner, a, b]
    rs = _list(ctx, data, shape, boxes, mode)
    _check_all(rs, data[2], shape, boxes)
    assert ctx.counter(13) == sum(_hits(shape, lo, hi) for lo, hi in boxes)       # duplicates counted
    assert _hits(shape, *a) == 1 and _hits(shape, *b) == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_thin_slabs_list_fewer_items_than_candidates(ctx, dtype):
    """(4, 40, 512): a tile is 8 rows, a plane 5 tiles.  The one-thick slab along the slowest axis is one whole plane and the
    one along the fastest axis crosses every row, so either hits every one of its candidate tiles (asserted from the mask:
    items == candidates for them); the slab along the middle axis hits one tile per plane out of 16 candidates.  The list
    with all three -- and every box with gaps of the single-call test -- lists strictly fewer items than candidates."""
    shape, mode = GAPS, H.EC
    data = B._case(ctx, shape, "ragged", dtype, mode)
    slabs = []
    for a in range(3):
        at = shape[a] // 3
        slabs.append((tuple(at if i == a else 0 for i in range(3)), tuple(at + 1 if i == a else shape[i] for i in range(3))))
    for boxes in ([slabs[0], slabs[2]], slabs, B.LOCAL_BOXES[GAPS]) + tuple([bx] for bx in B.LOCAL_BOXES[GAPS]):
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
    data = B._case(ctx, shape, "ragged", dtype, H.EC)
    full_box = ((0, 0, 0), shape)
    rs = _list(ctx, data, shape, [full_box] * 3, H.EC)
    assert ctx.counter(13) == 3 * (int(np.prod(shape)) // TILE) == 7680
    assert ctx.counter(14) < ctx.counter(13)
    for r in rs:
        assert B._same_dev(r.reshape(-1), data[2])


@pytest.mark.parametrize("case", B.LOCAL, ids=B._id)
def test_list_reads_only_the_union_of_the_hit_tiles(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = B._case(ctx, shape, kind, dtype, mode)
    n = int(np.prod(shape))
    boxes = B.LOCAL_BOXES[shape]
    hit = np.zeros(-(-n // TILE), bool)
    for lo, hi in boxes:
        hit |= B._hit_tiles(shape, lo, hi)[0]
    t = np.flatnonzero(hit)
    assert (~hit).any(), "every tile is hit by some box: nothing is poisoned"
    if shape in (GAPS, BIG):                           # tiles BETWEEN hit ones that no box of the list hits
        assert (~hit[t[0]:t[-1] + 1]).sum() >= 2
    pout, pix = B._poisoned(out, idx, n, hit, seed=3)
    rs = _list(ctx, data, shape, boxes, mode, out=pout, idx=pix)
    _check_all(rs, full, shape, boxes)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((5, 7, 9), (33, 65, 67)) and c[1] == "ragged"], ids=B._id)
def test_list_writes_only_its_outputs(ctx, case):
    """The outputs carved out of one arena, 64-byte guards between and around them (and the bytes up to the next 16-byte
    boundary behind an output): every byte that belongs to no output keeps its pattern."""
    import torch
    shape, kind, dtype, mode = case
    data = B._case(ctx, shape, kind, dtype, mode)
    tdt = data[6]
    es = 8 if dtype == np.float64 else 4
    boxes = B._corners(shape) + [B._odd_box(shape), ((0,) * len(shape), tuple(shape)), B._odd_box(shape)]
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


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((64 * 777 + 45,), (33, 65, 67)) and c[1] == "ragged"], ids=B._id)
def test_short_block_of_some_boxes_and_of_none(ctx, case):
    shape, kind, dtype, mode = case
    data = B._case(ctx, shape, kind, dtype, mode)
    n = int(np.prod(shape))
    full_end = n // 64 * 64
    assert n % 64
    flat = np.arange(n).reshape(shape)
    only, before = B._boxes(shape, 0, k=0)[-2:]        # inside the short block only / ending one element before it
    whole = ((0,) * len(shape), tuple(shape))
    first = ((0,) * len(shape), tuple(1 for _ in shape[:-1]) + (min(shape[-1], 50),))
    reach = lambda bx: int(flat[tuple(slice(l, h) for l, h in zip(*bx))].max()) >= full_end
    mixed = [before, only, first, whole]
    assert [reach(bx) for bx in mixed] == [False, True, False, True]
    none = [before, first, B._odd_box(shape)]
    assert not any(reach(bx) for bx in none)
    for boxes in (mixed, none):
        rs = _list(ctx, data, shape, boxes, mode)
        _check_all(rs, data[2], shape, boxes)


def _raw(ctx, out, cnt, n, tdt, eb, sf, dims, items, idx_ptr, mode, q, k=None, null=False):
    """items: (lo, hi, output pointer) per box; k (or None: their number) is what the call is told."""
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = (H.BoxItem * max(len(items), 1))()
    for it, (lo, hi, ptr) in zip(arr, items):
        for i, (l, h) in enumerate(zip(lo, hi)):
            it.lo[i], it.hi[i] = l, h
        it.d_out = ptr
    return ctx.lib.dctzhip_decompress_boxes(ctx.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
                                            int(cnt), idx_ptr, qp, n, H._dt(tdt), float(eb), float(sf), mode, len(dims),
                                            (C.c_size_t * len(dims))(*dims), len(items) if k is None else k,
                                            None if null else C.cast(arr, C.c_void_p))


# four boxes of (4, 40, 512); box 0 has 25 elements (24 of them a multiple of 16 bytes in either element type)
REF_BOXES = [((0, 0, 0), (1, 5, 5)), ((1, 3, 100), (3, 5, 200)), ((0, 39, 0), (4, 40, 512)), ((2, 7, 9), (3, 20, 60))]


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == GAPS], ids=B._id)
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = B._case(ctx, shape, kind, dtype, mode)
    n = int(np.prod(shape))
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    es = 8 if dtype == np.float64 else 4
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    sizes = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in REF_BOXES]
    starts = [0, 1024, 2048, 8192]                      # elements of one arena, 16-byte aligned
    arena = torch.empty(16384, dtype=tdt, device=ctx.device)
    B._ivw(arena).fill_(0x5A5A5A5A)
    sentinel = arena.clone()
    ptr = lambda i: arena.data_ptr() + starts[i] * es
    good = [(lo, hi, ptr(i)) for i, (lo, hi) in enumerate(REF_BOXES)]

    def swap(i, lo=None, hi=None, p=None):
        v = list(good)
        v[i] = (v[i][0] if lo is None else lo, v[i][1] if hi is None else hi, v[i][2] if p is None else p)
        return v

    def call(items=good, **kw):
        return _raw(ctx, cp, info.cnt, n, tdt, eb, info.sf, shape, items, idx.data_ptr(), mode, q, **kw)

    def untouched():
        assert B._same_dev(arena, sentinel)
        for k in out:
            bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
            assert torch.equal(bits(cp[k]), bits(out[k])), k

    def good_call():
        assert call() == H.OK
        for i, (lo, hi) in enumerate(REF_BOXES):
            r = arena[starts[i]:starts[i] + sizes[i]].view([h - l for l, h in zip(lo, hi)])
            assert B._same_dev(r, B._slice(full, shape, lo, hi)), (lo, hi)
        arena.copy_(sentinel)

    many = [good[0]] * (H.BOXES_MAX + 1)
    bin_at = cp["bin_index"].data_ptr() + (1 * 40 * 512 + 3 * 512) // 16 * 16          # bin ids that box 1 reads
    refused = [
        dict(k=0), dict(items=many), dict(null=True),
        dict(items=swap(2, hi=(4, 41, 512))),                                          # box 2 of 4: hi > dims
        dict(items=swap(1, p=ptr(1) + es)),                                            # box 1: misaligned output
        dict(items=swap(3, p=ptr(0) + (sizes[0] - 1) * es)),                           # outputs of boxes 0 and 3: one element in common
        dict(items=swap(1, p=bin_at)),                                                 # an output over bin_index
    ]
    assert (ptr(0) + (sizes[0] - 1) * es) % 16 == 0
    for kw in refused:
        assert call(**kw) == H.E_ARG, kw
        untouched()
        good_call()
    assert call(items=swap(2, hi=(4, 41, 512))) == H.E_ARG                             # the message names the box
    assert "box 2" in ctx.lib.dctzhip_last_error(ctx.h).decode()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == GAPS], ids=B._id)
def test_index_check_covers_the_hit_tiles_of_every_box(ctx, case):
    shape, kind, dtype, mode = case
    out, info, full, idx, eb, q, tdt = data = B._case(ctx, shape, kind, dtype, mode)
    boxes = [bx for bx in REF_BOXES]
    hits = [B._hit_tiles(shape, lo, hi)[0] for lo, hi in boxes]
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
    o, info_ = data[0], data[1]
    rc = _raw(ctx, o, info_.cnt, int(np.prod(shape)), tdt, eb, info_.sf, shape,
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


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_boxes_around_a_nan_tile(ctx, dtype, mode):
    """tests/nonfinite.py's poisoned tile: two boxes that straddle it and one that avoids it; NaN exactly where the full
    decode has NaN, the same bits everywhere else."""
    import torch
    shape = (33, 65, 67)
    n = int(np.prod(shape))
    x, bad = NF.make("nan_tile", n, dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out, info = ctx.compress(torch.from_numpy(x).to(ctx.device), 1e-3, mode)
    q = np.array(info.qtable[:]) if mode == H.QT else None
    full = ctx.decompress(out, info.cnt, n, tdt, 1e-3, info.sf, mode, qtable=q)
    idx, _ = ctx.ac_index(out, n)
    first, last = np.unravel_index(int(bad[0]) * 64, shape), np.unravel_index(min(int(bad[-1]) * 64 + 63, n - 1), shape)
    assert 2 <= int(first[0]) and int(last[0]) + 3 <= shape[0]
    boxes = [((int(first[0]) - 2, 3, 1), (int(last[0]) + 3, 60, 66)),
             ((int(first[0]) - 1, 0, 0), (int(last[0]) + 2, 65, 67)),
             ((0, 0, 0), (int(first[0]) - 1, 65, 67))]
    rs = ctx.decompress_boxes(out, info.cnt, shape, tdt, 1e-3, info.sf, boxes, idx, mode, qtable=q)
    for i, (r, (lo, hi)) in enumerate(zip(rs, boxes)):
        want = B._slice(full, shape, lo, hi).cpu().numpy()
        assert np.isnan(want).any() == (i < 2) and not np.isnan(want).all()
        assert NF.same_with_nans(r.cpu().numpy(), want), NF.describe_mismatch(r.cpu().numpy(), want)
