"""A list of boxes of the coarse decode of one array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one call (include/dctz_hip.h:
dctzhip_decompress_coarse_boxes_nd): a screenful of windows at zoom level f.

The yardstick is Context.decompress_coarse_nd, sliced, bit for bit (tests/test_gpu_coarse_decode.py holds that call to the
numpy low-band operator): no tolerance anywhere.  Every output of one list call is the slice, at non-contiguous destinations
too; the work list follows the hit stream tiles (dctzhip_debug_counter 13 against a count from a boolean mask over the block
grid); the grid-stride loop over the list; locality (everything outside the union of the hit tiles poisoned; for the DC-only
form everything outside each box's first-to-last DC words); output bounds (guards between and around the outputs of one
arena); the edges of k; the DC-only form without the other streams; a NaN block; the refusals, each followed by a good list
call on the same context; the index check; one call on a caller-selected stream directly behind its producers; the
kernel's name.

The workloads, shapes, boxes and the poisoning are those of the single-box test (tests/test_gpu_coarse_box_nd.py); the cached
cases -- each compressed once, its whole coarse arrays computed once and never written again -- are shared with it."""
import ctypes as C

import numpy as np
import pytest

from tests import nonfinite as NF
from tests import test_gpu_coarse_box_nd as CB
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

EDGE, FACTORS, TILE_BLKS = CB.EDGE, CB.FACTORS, CB.TILE_BLKS
BIG, GAPS2, GAPS3, RAGGED2, RAGGED3 = CB.BIG, CB.GAPS2, CB.GAPS3, CB.RAGGED2, CB.RAGGED3


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _list(ctx, data, shape, f, boxes, mode, out=None, idx=None, cnt=None, dsts=None):
    o, info, ix, eb, q, tdt, _ = data
    return ctx.decompress_coarse_boxes_nd(o if out is None else out, info.cnt if cnt is None else cnt, shape, tdt, eb, info.sf, f, boxes,
                                          index=ix if idx is None else idx, mode=mode, qtable=q, dsts=dsts)


def _hit(shape, f, lo, hi):
    return CB._hit_tiles(shape, f, lo, hi)[0]


def _hits(shape, f, boxes):
    """(box, hit stream tile) pairs of a list, from the boolean mask of the block grid; none for the DC-only form."""
    if EDGE[len(shape)] // f == 1:
        return 0
    return sum(int(_hit(shape, f, lo, hi).sum()) for lo, hi in boxes)


def _union(shape, f, boxes):
    hit = np.zeros_like(_hit(shape, f, *boxes[0]))
    for lo, hi in boxes:
        hit |= _hit(shape, f, lo, hi)
    return hit


def _kernel(shape, dtype, mode, f):
    K = EDGE[len(shape)] // f
    t = CB._tname(dtype)
    return f"k_ndcoarse_mbox_dc<{t}>" if K == 1 else f"k_ndcoarse_mbox<{t}, {mode}, {len(shape) - 1}, {K}>"


def _check_all(rs, whole, boxes, tag=None):
    assert len(rs) == len(boxes)
    for r, (lo, hi) in zip(rs, boxes):
        assert tuple(r.shape) == tuple(h - l for l, h in zip(lo, hi))
        assert CB._same_dev(r, CB._slice(whole, lo, hi)), (tag, lo, hi)


def _box_set(shape, f, seed):
    """The single-box test's set for the factor, plus one box given twice and one nested in another."""
    bx = CB._boxes(shape, f, seed)
    cd = CB._cext(shape, f)
    odd = CB._odd_box(cd)
    outer = CB._clamped(cd, [d // 5 for d in cd], [d - d // 5 for d in cd])
    inner = CB._clamped(cd, [l + 1 for l in outer[0]], [h - 1 for h in outer[1]])
    assert all(ol <= il < ih <= oh for ol, il, ih, oh in zip(outer[0], inner[0], inner[1], outer[1]))
    return bx + [odd, odd, outer, inner]


def _counters(ctx, shape, f, boxes):
    """Counter 13 is the hit pairs, within the host's bound; the DC-only form lists nothing."""
    items, wgs, bound = ctx.counter(13), ctx.counter(14), ctx.counter(15)
    assert items == _hits(shape, f, boxes), (f, items)
    assert items <= bound and wgs >= 1, (items, wgs, bound)
    if EDGE[len(shape)] // f == 1:
        assert items == 0 and bound == 0


# ---- every output is the slice -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CB.CASES, ids=CB._id)
def test_every_output_is_the_slice_of_the_coarse_decode(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    data = CB._case(ctx, shape, kind, dtype, mode)
    tdt = data[5]
    for f in FACTORS[len(shape)]:
        whole = data[6][f]
        boxes = _box_set(shape, f, seed=5)
        rs = _list(ctx, data, shape, f, boxes, mode)
        assert ctx.last_kernel(1) == _kernel(shape, dtype, mode, f)
        _counters(ctx, shape, f, boxes)
        _check_all(rs, whole, boxes, f)
        # destinations of the caller's, not next to each other and not in the order of the boxes
        sizes = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in boxes]
        slot = (max(sizes) + 19) // 4 * 4                                            # elements: 16-byte aligned in either type
        arena = torch.empty(slot * len(boxes), dtype=tdt, device=ctx.device)
        order = list(reversed(range(len(boxes))))
        dsts = [arena[slot * order[i]:slot * order[i] + sizes[i]] for i in range(len(boxes))]
        _check_all(_list(ctx, data, shape, f, boxes, mode, dsts=dsts), whole, boxes, f)
        # k = 1: the single call's bytes
        lo, hi = CB._odd_box(CB._cext(shape, f))
        (r,) = _list(ctx, data, shape, f, [(lo, hi)], mode)
        _counters(ctx, shape, f, [(lo, hi)])
        assert CB._same_dev(r, CB._box(ctx, data, shape, f, lo, hi, mode)), (f, lo, hi)


def test_workgroups_take_several_items(monkeypatch):
    """(256, 256, 160) at f = 2, fp64 EC: 2560 stream tiles.  The context of this test is created under DCTZHIP_WG_PER_CU=1, which
    the call honours as the single call does: at most one workgroup per CU, far fewer than items, the grid-stride loop over
    the list runs.  The whole coarse array and two more boxes: every tile is hit at least once."""
    import dctz_amd
    monkeypatch.setenv("DCTZHIP_WG_PER_CU", "1")
    c = dctz_amd.Context(0)
    try:
        dtype = np.float64
        data = CB._compressed(c, CB._input(BIG, "ragged", dtype), CB.EBS["ragged"], H.EC)
        cd = CB._cext(BIG, 2)
        boxes = [((0, 0, 0), cd), ((5, 50, 15), (10, 55, 75)), ((0, 0, 0), (cd[0], 1, cd[2]))]
        assert _union(BIG, 2, boxes).all() and _union(BIG, 2, boxes).size == 2560
        rs = _list(c, data, BIG, 2, boxes, H.EC)
        items, wgs = c.counter(13), c.counter(14)
        print(f"items {items}, workgroups {wgs}, bound {c.counter(15)}")
        assert items == _hits(BIG, 2, boxes) >= 2560 and items <= c.counter(15)
        assert 1 <= wgs < items
        assert c.last_kernel(1) == _kernel(BIG, dtype, H.EC, 2)
        _check_all(rs, data[6][2], boxes)
    finally:
        c.close()


# ---- locality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CB.LOCAL, ids=CB._id)
def test_list_reads_only_the_union_of_the_hit_tiles(ctx, case):
    """Everything of the three streams and the index outside the union of the hit tiles of LOCAL_BOXES[(shape, f)] is
    poisoned, candidate tiles between hit ones included; for the DC-only form everything outside the union of the boxes'
    first-to-last DC words.  Where the boxes together hit every tile the sub-lists that leave one without a hit run too."""
    import itertools
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = data = CB._case(ctx, shape, kind, dtype, mode)
    nblk = CB._nblk(shape)
    for f in FACTORS[len(shape)]:
        K = EDGE[len(shape)] // f
        boxes = CB.LOCAL_BOXES[(shape, f)]
        if K == 1:
            keep = np.zeros(nblk, bool)
            for lo, hi in boxes:
                _, _, _, bfirst, blast = CB._hit_tiles(shape, f, lo, hi)
                keep[bfirst:blast + 1] = True
            assert not keep.all()
            pout, pix = CB._poisoned(out, idx, nblk, np.zeros_like(_hit(shape, f, *boxes[0])), seed=3, dc_keep=keep)
            _check_all(_list(ctx, data, shape, f, boxes, mode, out=pout, idx=pix), coarse[f], boxes, f)
            continue
        lists = [boxes]
        if _union(shape, f, boxes).all():
            subs = [list(s) for r in range(len(boxes) - 1, 0, -1) for s in itertools.combinations(boxes, r)]
            lists = [s for s in subs if not _union(shape, f, s).all()]
        for bx in lists:
            hit = _union(shape, f, bx)
            assert not hit.all(), "every tile is hit by some box: nothing is poisoned"
            t = np.flatnonzero(hit)
            if shape in (GAPS2, GAPS3):                 # tiles BETWEEN hit ones that no box of the list hits
                assert (~hit[t[0]:t[-1] + 1]).sum() >= 2, (f, bx)
            pout, pix = CB._poisoned(out, idx, nblk, hit, seed=3)
            _check_all(_list(ctx, data, shape, f, bx, mode, out=pout, idx=pix), coarse[f], bx, f)


# ---- output bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CB.GUARDED, ids=CB._id)
def test_list_writes_only_its_outputs(ctx, case):
    """The outputs carved out of one arena, 64-byte guards between and around them (and the bytes up to the next 16-byte
    boundary behind an output): every byte that belongs to no output keeps its pattern."""
    import torch
    shape, kind, dtype, mode = case
    data = CB._case(ctx, shape, kind, dtype, mode)
    tdt = data[5]
    es = 8 if dtype == np.float64 else 4
    for f in FACTORS[len(shape)]:
        K = EDGE[len(shape)] // f
        cd = CB._cext(shape, f)
        boxes = CB._corners(cd) + [CB._odd_box(cd), CB._aligned(cd, CB._nb(shape), K), CB._far_corner(cd), ((0,) * len(cd), cd), CB._odd_box(cd)]
        at, spans = 64, []
        for lo, hi in boxes:
            nb = int(np.prod([h - l for l, h in zip(lo, hi)])) * es
            spans.append((at, nb))
            at = (at + nb + 15) // 16 * 16 + 64
        arena = torch.full((at,), 0x5A, dtype=torch.uint8, device=ctx.device)
        assert arena.data_ptr() % 16 == 0
        dsts = [arena[a:a + nb].view(tdt) for a, nb in spans]
        _check_all(_list(ctx, data, shape, f, boxes, mode, dsts=dsts), data[6][f], boxes, f)
        mine = torch.zeros(at, dtype=torch.bool, device=ctx.device)
        for a, nb in spans:
            mine[a:a + nb] = True
        assert bool((arena[~mine] == 0x5A).all()), f
        assert int((~mine).sum()) >= 64 * (len(boxes) + 1)


# ---- the edges of k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 512), (16, 16, 32)], ids=["64x512", "16x16x32"])
def test_as_many_boxes_as_a_call_takes(ctx, shape):
    """DCTZHIP_BOXES_MAX one-cell boxes in one call, at every factor; k = 0 and one more than the maximum are refused."""
    import torch
    dtype, mode = np.float64, H.EC
    data = CB._case(ctx, shape, "ragged", dtype, mode)
    for f in FACTORS[len(shape)]:
        cd = CB._cext(shape, f)
        ncell = int(np.prod(cd))
        cells = [np.unravel_index((i * 7919) % ncell, cd) for i in range(H.BOXES_MAX)]
        boxes = [(tuple(int(v) for v in c), tuple(int(v) + 1 for v in c)) for c in cells]
        arena = torch.empty(2 * H.BOXES_MAX, dtype=data[5], device=ctx.device)          # an fp64 cell per 16 bytes
        dsts = [arena[2 * i:2 * i + 1] for i in range(H.BOXES_MAX)]
        rs = _list(ctx, data, shape, f, boxes, mode, dsts=dsts)
        _counters(ctx, shape, f, boxes)
        got = arena[::2]                                                                 # (the outputs are views of the arena)
        flat = data[6][f].reshape(-1)
        want = flat[torch.tensor([(i * 7919) % ncell for i in range(H.BOXES_MAX)], device=ctx.device)]
        assert CB._same_dev(got, want), f
        with pytest.raises(H.DctzHipError):
            _list(ctx, data, shape, f, [], mode)
        with pytest.raises(H.DctzHipError):
            _list(ctx, data, shape, f, boxes + boxes[:1], mode, dsts=dsts + [torch.empty(1, dtype=data[5], device=ctx.device)])
        _check_all(_list(ctx, data, shape, f, boxes[:3], mode), data[6][f], boxes[:3], f)


# ---- the DC-only form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CB.CASES if c[0] in (RAGGED2, RAGGED3, GAPS2, GAPS3) and c[1] == "ragged"], ids=CB._id)
def test_dc_only_form_needs_the_dc_stream_alone(ctx, case):
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = CB._case(ctx, shape, kind, dtype, mode)
    f = EDGE[len(shape)]
    boxes = _box_set(shape, f, seed=7)
    rs = ctx.decompress_coarse_boxes_nd({"dc": out["dc"]}, 0, shape, tdt, eb, info.sf, f, boxes, index=None, mode=mode, qtable=q)
    _check_all(rs, coarse[f], boxes)
    assert ctx.last_kernel(1) == f"k_ndcoarse_mbox_dc<{CB._tname(dtype)}>"
    assert ctx.counter(13) == 0 and ctx.counter(15) == 0 and ctx.counter(14) >= 1


# ---- a NaN block -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RAGGED2, RAGGED3], ids=["45x77", "13x22x35"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [H.EC, H.QT], ids=["EC", "QT"])
def test_boxes_around_a_nan_block(ctx, shape, dtype, mode):
    """A NaN in one block: a box that straddles the block is NaN exactly where the whole-array coarse call is NaN and keeps the
    same bits everywhere else (tests/nonfinite.py's rule); a box that ends in front of the block has no NaN."""
    x = CB._input(shape, "ragged", dtype)
    at = tuple(d // 2 for d in shape)
    x[at] = np.nan
    out, info, idx, eb, q, tdt, coarse = CB._compressed(ctx, x, 1e-3, mode)
    e = EDGE[len(shape)]
    for f in FACTORS[len(shape)]:
        K = e // f
        cd = CB._cext(shape, f)
        boxes = [(tuple(max(0, a // f - K - 1) for a in at), tuple(min(d, a // f + K + 2) for a, d in zip(at, cd))),
                 ((0,) * len(shape), tuple(a // e * K for a in at))]                     # ends in front of the NaN's block on every axis
        rs = ctx.decompress_coarse_boxes_nd(out, info.cnt, shape, tdt, eb, info.sf, f, boxes, index=idx, mode=mode, qtable=q)
        for i, (r, (lo, hi)) in enumerate(zip(rs, boxes)):
            want = CB._slice(coarse[f], lo, hi).cpu().numpy()
            assert np.isnan(want).any() == (i == 0) and not np.isnan(want).all(), (f, i)
            assert NF.same_with_nans(r.cpu().numpy(), want), (f, i, NF.describe_mismatch(r.cpu().numpy(), want))


# ---- refusals and the index check --------------------------------------------------------------------------------------------
def _raw(ctx, out, cnt, tdt, eb, sf, dims, f, items, idx_ptr, mode, q, k=None, null=False, bin_ptr=None):
    """items: (lo, hi, output pointer) per box; k (or None: their number) is what the call is told."""
    qp = q.ctypes.data_as(C.c_void_p) if q is not None else None
    arr = (H.BoxItem * max(len(items), 1))()
    for it, (lo, hi, ptr) in zip(arr, items):
        for i, (l, h) in enumerate(zip(lo, hi)):
            it.lo[i], it.hi[i] = l, h
        it.d_out = ptr
    return ctx.lib.dctzhip_decompress_coarse_boxes_nd(ctx.h, out["bin_index"].data_ptr() if bin_ptr is None else bin_ptr, out["dc"].data_ptr(),
                                                      out["ac_exact"].data_ptr(), int(cnt), idx_ptr, qp, len(dims), (C.c_size_t * len(dims))(*dims),
                                                      H._dt(tdt), float(eb), float(sf), mode, int(f), len(items) if k is None else k,
                                                      None if null else C.cast(arr, C.c_void_p))


# at factor 2.  Box 0 is the single-box test's (three hit tiles with gaps between them); box 1 has 25 cells (24 of them a
# multiple of 16 bytes in either element type); box 2 hits tiles that no other box of the list hits
REF_BOXES = {GAPS2: [((0, 0), (12, 8)), ((4, 300), (9, 305)), ((8, 500), (12, 772)), ((2, 7), (3, 60))],
             GAPS3: [((0, 4, 10), (6, 6, 20)), ((0, 0, 0), (1, 5, 5)), ((0, 31, 0), (6, 32, 128)), ((1, 7, 9), (2, 10, 60))]}


@pytest.mark.parametrize("case", [c for c in CB.CASES if c[0] in REF_BOXES], ids=CB._id)
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx, case):
    import torch
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = CB._case(ctx, shape, kind, dtype, mode)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32)
    es = 8 if dtype == np.float64 else 4
    nd = len(shape)
    cp = {k: v.clone() for k, v in out.items()}         # a refusal that did not happen must not damage the cached case
    ref = REF_BOXES[shape]
    cd = CB._cext(shape, 2)
    sizes = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in ref]
    starts = [0, 1024, 2048, 8192]                      # elements of one arena, 16-byte aligned
    assert sizes[1] == 25 and all(s + z <= e for s, z, e in zip(starts, sizes, starts[1:] + [16384]))
    arena = torch.empty(16384, dtype=tdt, device=ctx.device)
    CB._ivw(arena).fill_(0x5A5A5A5A)
    sentinel = arena.clone()
    ptr = lambda i: arena.data_ptr() + starts[i] * es
    good = [(lo, hi, ptr(i)) for i, (lo, hi) in enumerate(ref)]

    def swap(i, lo=None, hi=None, p=None):
        v = list(good)
        v[i] = (v[i][0] if lo is None else lo, v[i][1] if hi is None else hi, p if p is not None else v[i][2])
        return v

    def call(items=good, f=2, qq=q, **kw):
        return _raw(ctx, cp, info.cnt, tdt, eb, info.sf, shape, f, items, idx.data_ptr(), mode, qq, **kw)

    def untouched():
        assert CB._same_dev(arena, sentinel)
        for k in out:
            bits = (lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v)
            assert torch.equal(bits(cp[k]), bits(out[k])), k

    def good_call():
        assert call() == H.OK
        for i, (lo, hi) in enumerate(ref):
            r = arena[starts[i]:starts[i] + sizes[i]].view([h - l for l, h in zip(lo, hi)])
            assert CB._same_dev(r, CB._slice(coarse[2], lo, hi)), (lo, hi)
        arena.copy_(sentinel)

    good_call()
    t0_0 = CB._hit_tiles(shape, 2, *ref[0])[1]
    bin_at = cp["bin_index"].data_ptr() + 4096 * t0_0   # bin ids that box 0 reads: its first candidate stream tile
    past = tuple(cd[i] + 1 if i == nd - 1 else ref[2][1][i] for i in range(nd))
    refused = [
        dict(k=0), dict(items=[good[0]] * (H.BOXES_MAX + 1)), dict(null=True),
        dict(f=3), dict(f=1), dict(f=16), dict(f=0),                                   # no such factor
        dict(items=swap(2, hi=past)),                                                  # box 2 of 4: one past the coarse extent
        dict(items=swap(2, hi=tuple(shape))),                                          # ... the extent in ELEMENTS
        dict(items=swap(1, lo=ref[1][1])),                                             # box 1: empty
        dict(items=[good[0], (good[1][0], good[1][1], None)] + good[2:]),              # box 1: null output
        dict(items=swap(1, p=ptr(1) + es)),                                            # box 1: misaligned output
        dict(items=swap(3, p=ptr(1) + (sizes[1] - 1) * es)),                           # outputs of boxes 1 and 3: one element in common
        dict(items=swap(1, p=bin_at)),                                                 # an output over bin ids a box reads
    ]
    if nd == 3:
        refused.append(dict(f=8))
    if mode == H.QT:
        refused.append(dict(qq=None))                                                  # QT without its table
        refused.append(dict(qq=None, f=EDGE[nd], items=[((0,) * nd, (1,) * nd, ptr(0))]))
    assert (ptr(1) + (sizes[1] - 1) * es) % 16 == 0
    for kw in refused:
        assert call(**kw) == H.E_ARG, kw
        untouched()
        good_call()
    # the DC-only form: an output over a DC word that another box reads
    one = [((0,) * nd, (1,) * nd, ptr(0)), ((0,) * nd, (1,) * (nd - 1) + (2,), cp["dc"].data_ptr())]
    assert call(f=EDGE[nd], items=one) == H.E_ARG
    untouched()
    good_call()
    for kw, i in ((dict(items=swap(2, hi=past)), 2), (dict(items=swap(1, p=ptr(1) + es)), 1), (dict(items=swap(1, lo=ref[1][1])), 1)):
        assert call(**kw) == H.E_ARG                                                   # the message names the box
        assert f"box {i}" in ctx.lib.dctzhip_last_error(ctx.h).decode(), kw
    good_call()


@pytest.mark.parametrize("case", [c for c in CB.CASES if c[0] in REF_BOXES], ids=CB._id)
def test_index_check_covers_the_hit_tiles_of_every_box(ctx, case):
    shape, kind, dtype, mode = case
    out, info, idx, eb, q, tdt, coarse = data = CB._case(ctx, shape, kind, dtype, mode)
    boxes = list(REF_BOXES[shape])
    hits = [_hit(shape, 2, lo, hi) for lo, hi in boxes]
    anyhit = hits[0] | hits[1] | hits[2] | hits[3]
    others = hits[0] | hits[1] | hits[3]
    own = np.flatnonzero(hits[2] & ~others & ~np.roll(others, 1))                       # neither idx[t] nor idx[t + 1] of another box's tile
    own = [int(t) for t in own if not others[t + 1:t + 2].any()]
    assert own

    def good_call():
        _check_all(_list(ctx, data, shape, 2, boxes, mode), coarse[2], boxes)

    t = own[-1]
    ix = idx.clone()
    ix[t + 1] += 1                                     # tile t of box 2 alone: its flags no longer number idx[t + 1] - idx[t]
    rs = _list(ctx, data, shape, 2, boxes, mode)
    rc = _raw(ctx, out, info.cnt, tdt, eb, info.sf, shape, 2, [(lo, hi, r.data_ptr()) for (lo, hi), r in zip(boxes, rs)], ix.data_ptr(), mode,
              None if q is None else np.ascontiguousarray(q, dtype=np.float64 if dtype == np.float64 else np.float32))
    assert rc == H.E_ARG
    good_call()
    # the same at entries that belong to no listed tile, candidates between hit ones included: not read
    free = [t for t in range(1, anyhit.size) if not anyhit[t] and not anyhit[t - 1]]
    assert free
    for t in free[:3]:
        ix = idx.clone()
        ix[t] += 1
        _check_all(_list(ctx, data, shape, 2, boxes, mode, idx=ix), coarse[2], boxes)
    # ac_count one short of what the last hit tile of the list needs
    need = int(idx[int(np.flatnonzero(anyhit)[-1]) + 1])
    assert need > 0
    with pytest.raises(H.DctzHipError):
        _list(ctx, data, shape, 2, boxes, mode, cnt=need - 1)
    good_call()
    _check_all(_list(ctx, data, shape, 2, boxes, mode, cnt=need), coarse[2], boxes)


# ---- stream order ------------------------------------------------------------------------------------------------------------
def test_list_on_a_caller_stream_behind_its_producers(ctx):
    """compress_nd, ac_index and the list call on a stream of the caller's, nothing of the test's between them."""
    import torch
    shape, dtype, mode, f = RAGGED3, np.float64, H.EC, 2
    data = CB._case(ctx, shape, "ragged", dtype, mode)
    cd = CB._cext(shape, f)
    boxes = [CB._odd_box(cd), CB._far_corner(cd), ((0,) * 3, cd)]
    xh = torch.from_numpy(CB._input(shape, "ragged", dtype)).pin_memory()
    s = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(s):
        x = xh.to(ctx.device, non_blocking=True)
        out, info = ctx.compress_nd(x, CB.EBS["ragged"], mode)
        idx, tot = ctx.ac_index(out, 64 * CB._nblk(shape))
        rs = ctx.decompress_coarse_boxes_nd(out, info.cnt, shape, CB._tdt(dtype), CB.EBS["ragged"], info.sf, f, boxes, index=idx, mode=mode)
        keep = [r.clone() for r in rs]
    s.synchronize()
    assert tot == info.cnt
    _check_all(keep, data[6][f], boxes)
    ctx._bind_stream()                                  # back on the default stream for the tests behind this one
