"""Every refusal of the box, range and mask entry points keeps its return code and its dctzhip_last_error text.

A table of single-fault calls through the raw C ABI -- one good argument set per entry point, element type and shape, one
argument wrong per row -- against tests/golden/refusal_texts.json, a list of {call, fault, code, text} recorded once from
the library (python -m tests.test_gpu_refusal_texts [path] writes it).  Host code that is folded, split or moved must leave
the table as it is.  After the last refusal of an entry point a good call on the same context returns DCTZHIP_OK.

All buffers of a call are carved out of one arena in a fixed order, so which range sorts first -- and with it the item
that a message about overlapping buffers names -- does not depend on the allocator.  Shapes: flat 8229 elements seen as
3 x 2743 (three stream tiles, a 37-element short block); tiled 72 x 80 (90 blocks, two stream tiles) and the ragged
13 x 22 x 35 (216 blocks, four stream tiles).  EC mode; QT only for the row of the missing table.  The refusal of a list
that may hit more than 2^24 tiles is not here: its buffers are larger than a test should allocate."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from tests import workloads as W
from dctz_amd import hip as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_texts.json")
EB = 1e-3
FLAT = (3, 2743)
TILED = [(72, 80), (13, 22, 35)]
# four boxes per shape; box 0 has 25 elements (24 of them a multiple of 16 bytes in either element type)
BOXES = {
    FLAT: [((0, 0), (1, 25)), ((1, 100), (3, 200)), ((0, 2700), (3, 2743)), ((2, 7), (3, 60))],
    (72, 80): [((0, 0), (5, 5)), ((8, 16), (24, 40)), ((0, 79), (72, 80)), ((30, 7), (41, 60))],
    (13, 22, 35): [((0, 0, 0), (1, 5, 5)), ((1, 3, 10), (3, 5, 20)), ((0, 21, 0), (13, 22, 35)), ((2, 7, 9), (3, 20, 30))],
}
RANGE = (4000, 8229)                                   # tiles 0 to 2 and the short block
DECODERS = {"dctzhip_decompress_range": False, "dctzhip_decompress_box": False, "dctzhip_decompress_boxes": False,
            "dctzhip_decompress_box_nd": True, "dctzhip_decompress_boxes_nd": True}
MASKS = {"dctzhip_mask_build": False, "dctzhip_compress_masked": False, "dctzhip_mask_build_nd": True, "dctzhip_compress_masked_nd": True}
VARIANTS = [(name, shape, dt) for name, tiled in {**DECODERS, **MASKS}.items() for shape in (TILED if tiled else [FLAT])
            for dt in (np.float32, np.float64)]


def _label(v):
    name, shape, dt = v
    return f"{name}-{np.dtype(dt).name}-{'x'.join(map(str, shape))}"


@pytest.fixture(scope="module")
def ctx():
    import dctz_amd
    c = dctz_amd.Context(0)
    yield c
    c.close()


def _sizes(shape):
    return [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in BOXES[shape]]


def _first_tile(shape, tiled, lo):
    """The first candidate stream tile of a box that starts at lo."""
    if not tiled:
        return int(np.ravel_multi_index(lo, shape)) // 4096
    e = 8 if len(shape) == 2 else 4
    return int(np.ravel_multi_index([l // e for l in lo], [-(-d // e) for d in shape])) // 64


class Buffers:
    """The arena of one variant and the good arguments of its call."""

    def __init__(self, ctx, shape, tiled, dtype):
        import torch
        self.shape, self.tiled = shape, tiled
        self.tdt = torch.float64 if dtype == np.float64 else torch.float32
        self.es = es = np.dtype(dtype).itemsize
        self.n = n = int(np.prod(shape))
        self.n_lin = n_lin = ctx.nd_blocks(shape) * 64 if tiled else n
        # (pad: room in front of the array for a filled copy that runs into it from below)
        parts = [("pad", n * es), ("x", n * es), ("bin", n_lin), ("dc", (n_lin + 63) // 64 * 4), ("ac", n_lin * 4),
                 ("index", int(ctx.lib.dctzhip_ac_index_len(n_lin)) * 4)]
        parts += [(f"out{i}", z * es) for i, z in enumerate(_sizes(shape))]
        parts += [("range", (RANGE[1] - RANGE[0]) * es), ("mask", (n + 63) // 64 * 8), ("filled", n * es)]
        self.at, end = {}, 0
        for name, nbytes in parts:
            self.at[name] = end
            end = (end + nbytes + 63) // 64 * 64 + 64
        self.arena = torch.zeros(end, dtype=torch.uint8, device=ctx.device)
        assert self.arena.data_ptr() % 256 == 0
        view = lambda name, nbytes, dt: self.arena[self.at[name]:self.at[name] + nbytes].view(dt)
        x = view("x", n * es, self.tdt)
        x.copy_(torch.from_numpy(W.ragged(n, dtype, scale=37.0)))
        self.out = {"bin_index": view("bin", n_lin, torch.uint8), "dc": view("dc", (n_lin + 63) // 64 * 4, torch.float32),
                    "ac_exact": view("ac", n_lin * 4, torch.float32)}
        if tiled:
            _, self.info = ctx.compress_nd(x.view(shape), EB, H.EC, out=self.out)
        else:
            _, self.info = ctx.compress(x, EB, H.EC, out=self.out)
        assert self.info.cnt > 0
        tot = C.c_uint32(0)
        assert ctx.lib.dctzhip_ac_index(ctx.h, self.p("bin"), n_lin, self.p("index"), C.byref(tot)) == H.OK and tot.value == self.info.cnt

    def p(self, name):
        return self.arena.data_ptr() + self.at[name]


def _arr(v):
    return None if v is None else (C.c_size_t * max(len(v), 1))(*v)


def _decode_call(ctx, name, a):
    """The raw call of a decoder from the argument dictionary a."""
    lib = ctx.lib
    head = (a["h"], a["bin"], a["dc"], a["ac"], a["cnt"], a["index"], a["q"])
    tail = (a["dtype"], EB, a["sf"], a["mode"])
    if name == "dctzhip_decompress_range":
        return lib.dctzhip_decompress_range(*head, a["n"], *tail, a["lo"], a["hi"], a["out"])
    items = None
    if name.startswith("dctzhip_decompress_boxes") and a["items"] is not None:
        items = (H.BoxItem * max(len(a["items"]), 1))()
        for it, (lo, hi, ptr) in zip(items, a["items"]):
            for i, (l, h) in enumerate(zip(lo, hi)):
                it.lo[i], it.hi[i] = l, h
            it.d_out = ptr
        items = C.cast(items, C.c_void_p)
    if name == "dctzhip_decompress_box":
        return lib.dctzhip_decompress_box(*head, a["n"], *tail, a["ndim"], _arr(a["dims"]), _arr(a["lo"]), _arr(a["hi"]), a["out"])
    if name == "dctzhip_decompress_boxes":
        return lib.dctzhip_decompress_boxes(*head, a["n"], *tail, a["ndim"], _arr(a["dims"]), a["k"], items)
    if name == "dctzhip_decompress_box_nd":
        return lib.dctzhip_decompress_box_nd(*head, a["ndim"], _arr(a["dims"]), *tail, _arr(a["lo"]), _arr(a["hi"]), a["out"])
    return lib.dctzhip_decompress_boxes_nd(*head, a["ndim"], _arr(a["dims"]), *tail, a["k"], items)


def _decode_table(ctx, name, b):
    """(good arguments, [(fault, changed arguments)]) of a decoder."""
    shape, tiled, es = b.shape, b.tiled, b.es
    boxes, sizes = BOXES[shape], _sizes(shape)
    good = dict(h=ctx.h, bin=b.p("bin"), dc=b.p("dc"), ac=b.p("ac"), cnt=int(b.info.cnt), index=b.p("index"), q=None, n=b.n,
                dtype=H._dt(b.tdt), sf=float(b.info.sf), mode=H.EC, ndim=len(shape), dims=tuple(shape))
    faults = [("bad dtype", dict(dtype=2)), ("bad mode", dict(mode=2)),
              ("bin_index NULL", dict(bin=None)), ("DC NULL", dict(dc=None)), ("AC_exact NULL", dict(ac=None)), ("index NULL", dict(index=None)),
              ("bin_index misaligned", dict(bin=b.p("bin") + 8)), ("DC misaligned", dict(dc=b.p("dc") + 2)),
              ("AC_exact misaligned", dict(ac=b.p("ac") + 2)), ("index misaligned", dict(index=b.p("index") + 2)),
              ("QT without its table", dict(mode=H.QT))]
    if tiled:
        faults += [("ndims 1", dict(ndim=1, dims=shape[:1])), ("ndims 4", dict(ndim=4, dims=tuple(shape) + (1,) * (4 - len(shape)))),
                   ("dims NULL", dict(dims=None)), ("an extent of 0", dict(dims=(0,) + tuple(shape[1:])))]
    else:
        faults += [("n = 0", dict(n=0))]
    if name != "dctzhip_decompress_range" and not tiled:
        faults += [("ndim 0", dict(ndim=0)), ("ndim 5", dict(ndim=5, dims=tuple(shape) + (1, 1, 1))), ("dims NULL", dict(dims=None)),
                   ("product of dims is not n", dict(dims=(shape[0], shape[1] + 1)))]
    one = 1                                            # the box of the single-box calls, and the one whose output goes astray
    bin_read = b.p("bin") + 4096 * _first_tile(shape, tiled, boxes[one][0]) + 16
    if name == "dctzhip_decompress_range":
        good.update(lo=RANGE[0], hi=RANGE[1], out=b.p("range"))
        faults += [("lo >= hi", dict(lo=RANGE[1], hi=RANGE[1])), ("hi > n", dict(hi=b.n + 1)),
                   ("output NULL", dict(out=None)), ("output misaligned", dict(out=b.p("range") + es)),
                   ("output over bin ids the call reads", dict(out=b.p("bin") + 4096 * (RANGE[0] // 4096) + 16))]
    elif "boxes" not in name:
        lo, hi = boxes[one]
        good.update(lo=lo, hi=hi, out=b.p(f"out{one}"))
        faults += [("lo NULL", dict(lo=None)), ("hi NULL", dict(hi=None)),
                   ("lo >= hi", dict(lo=hi[:1] + lo[1:])), ("hi > dim", dict(hi=hi[:-1] + (shape[-1] + 1,))),
                   ("output NULL", dict(out=None)), ("output misaligned", dict(out=b.p(f"out{one}") + es)),
                   ("output over bin ids the box reads", dict(out=bin_read))]
    else:
        items = [(lo, hi, b.p(f"out{i}")) for i, (lo, hi) in enumerate(boxes)]

        def swap(i, lo=None, hi=None, p=0):
            v = list(items)
            v[i] = (v[i][0] if lo is None else lo, v[i][1] if hi is None else hi, v[i][2] if p == 0 else p)
            return v

        lo2, hi2 = boxes[2]
        assert (b.p("out0") + (sizes[0] - 1) * es) % 16 == 0
        good.update(k=len(items), items=items)
        faults += [("k = 0", dict(k=0)), ("k = DCTZHIP_BOXES_MAX + 1", dict(k=H.BOXES_MAX + 1, items=[items[0]] * (H.BOXES_MAX + 1))),
                   ("boxes NULL", dict(items=None)),
                   ("box 2 of 4: lo >= hi", dict(items=swap(2, lo=hi2[:1] + lo2[1:]))),
                   ("box 2 of 4: hi > dim", dict(items=swap(2, hi=hi2[:-1] + (shape[-1] + 1,)))),
                   ("box 2 of 4: output NULL", dict(items=swap(2, p=None))),
                   ("box 1 of 4: output misaligned", dict(items=swap(1, p=b.p("out1") + es))),
                   ("outputs of boxes 0 and 3 share one element", dict(items=swap(3, p=b.p("out0") + (sizes[0] - 1) * es))),
                   ("output of box 1 over bin ids it reads", dict(items=swap(1, p=bin_read)))]
    return good, faults


def _mask_call(ctx, name, a):
    lib = ctx.lib
    miss = C.byref(a["miss"]) if a["miss"] is not None else None
    count = C.byref(a["count"]) if a["count"] is not None else None
    geo = (a["ndim"], _arr(a["dims"])) if name.endswith("_nd") else (a["n"],)
    if name.startswith("dctzhip_mask_build"):
        return getattr(lib, name)(a["h"], a["x"], *geo, a["dtype"], miss, a["mask"], a["filled"], count)
    return getattr(lib, name)(a["h"], a["x"], *geo, a["dtype"], a["eb"], a["mode"], miss, a["bin"], a["dc"], a["ac"], a["mask"], a["filled"],
                              C.byref(a["info"]), count)


def _mask_table(ctx, name, b):
    """(good arguments, [(fault, changed arguments)]) of a mask call."""
    shape, tiled, es = b.shape, b.tiled, b.es
    good = dict(h=ctx.h, x=b.p("x"), n=b.n, ndim=len(shape), dims=tuple(shape), dtype=H._dt(b.tdt), miss=H.Missing(H.MISS_NAN, 0.0, 0.0),
                mask=b.p("mask"), filled=b.p("filled"), count=C.c_uint64(0), eb=EB, mode=H.EC, bin=b.p("bin"), dc=b.p("dc"), ac=b.p("ac"),
                info=H.CompressInfo())
    inf, nan = float("inf"), float("nan")
    faults = [("bad dtype", dict(dtype=2)),
              ("rule NULL", dict(miss=None)), ("flags 0", dict(miss=H.Missing(0, 0.0, 0.0))),
              ("an unknown flag bit", dict(miss=H.Missing(H.MISS_NAN | 32, 0.0, 0.0))),
              ("a NaN value", dict(miss=H.Missing(H.MISS_VALUE, nan, 0.0))),
              ("a limit of 0", dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, 0.0))), ("a limit of infinity", dict(miss=H.Missing(H.MISS_ABS_GE, 0.0, inf))),
              ("array NULL", dict(x=None)), ("mask NULL", dict(mask=None)), ("count NULL", dict(count=None)),
              ("array misaligned", dict(x=b.p("x") + es)), ("mask misaligned", dict(mask=b.p("mask") + 4)),
              ("d_filled misaligned", dict(filled=b.p("filled") + es)),
              ("d_filled overlaps the mask", dict(mask=b.p("filled") + 64)),
              ("d_filled overlaps the array by two elements", dict(filled=b.p("x") - (b.n - 2) * es // 16 * 16)),
              ("the mask inside the array", dict(mask=b.p("x") + 64))]
    if tiled:
        faults += [("ndims 1", dict(ndim=1, dims=shape[:1])), ("ndims 4", dict(ndim=4, dims=tuple(shape) + (1,) * (4 - len(shape)))),
                   ("dims NULL", dict(dims=None)), ("an extent of 0", dict(dims=(0,) + tuple(shape[1:])))]
    else:
        faults += [("n = 0", dict(n=0))]
    if name.startswith("dctzhip_compress_masked"):
        faults += [("bad mode", dict(mode=2)), ("eb < 1e-6", dict(eb=1e-7)),
                   ("bin_index NULL", dict(bin=None)), ("DC NULL", dict(dc=None)), ("AC_exact NULL", dict(ac=None)),
                   ("bin_index misaligned", dict(bin=b.p("bin") + 8)), ("DC misaligned", dict(dc=b.p("dc") + 4)),
                   ("AC_exact misaligned", dict(ac=b.p("ac") + 4)),
                   ("d_filled is the array", dict(filled=b.p("x"))), ("the mask over bin_index", dict(mask=b.p("bin"))),
                   ("d_filled over AC_exact", dict(filled=b.p("ac")))]
    return good, faults


def _rows(ctx, variant):
    """The rows of one variant as they come out of the library, then one good call."""
    name, shape, dtype = variant
    tiled = {**DECODERS, **MASKS}[name]
    b = Buffers(ctx, shape, tiled, dtype)
    table, call = (_decode_table, _decode_call) if name in DECODERS else (_mask_table, _mask_call)
    good, faults = table(ctx, name, b)
    assert len({f for f, _ in faults}) == len(faults)
    rows = []
    for fault, changed in faults:
        code = call(ctx, name, {**good, **changed})
        rows.append({"call": _label(variant), "fault": fault, "code": int(code), "text": ctx.lib.dctzhip_last_error(ctx.h).decode()})
    assert call(ctx, name, good) == H.OK, ctx.lib.dctzhip_last_error(ctx.h).decode()
    return rows


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_lists_the_calls_of_the_table(golden):
    assert sorted({r["call"] for r in golden}) == sorted(_label(v) for v in VARIANTS)
    assert all(r["code"] in (H.E_ARG, H.E_BOUND) and r["text"] for r in golden)


@pytest.mark.parametrize("variant", VARIANTS, ids=_label)
def test_every_refusal_keeps_its_code_and_text(ctx, golden, variant):
    want = [r for r in golden if r["call"] == _label(variant)]
    got = _rows(ctx, variant)
    assert [r["fault"] for r in got] == [r["fault"] for r in want]
    for g, w in zip(got, want):
        assert (g["code"], g["text"]) == (w["code"], w["text"]), g["fault"]


if __name__ == "__main__":
    import dctz_amd
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    c = dctz_amd.Context(0)
    rows = [r for v in VARIANTS for r in _rows(c, v)]
    c.close()
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows -> {path}")
