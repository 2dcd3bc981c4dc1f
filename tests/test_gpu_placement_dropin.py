"""Placement of the drop-in's host buffers ("Placement, what is pinned").  var->buf, var_r->buf and the
container bytes of the other drop-in tests are numpy allocations of their own; an HPC caller hands over a field out of the
middle of a larger array.  Here every caller-owned array starts ONE ELEMENT into a larger one -- 4 (mod 8) in fp32, 8 (mod 16)
in fp64 -- and the container bytes ONE BYTE into theirs, for dctz_compress / dctz_decompress (EC and QT builds, the reference's
zlib tail and DCTZ_ZLIB_GPU=1), the batch pair and every partial reader.  Containers are built from the oracle's streams
(tests/containers.py); a whole decode, a range and a box are the oracle's decode and its slices, every other reader gives what
the same call gives on buffers of their own, bit for bit; the element (the byte) on either side of every output is unchanged.

The pipelined paths (DCTZ_PIPELINE_*) start at sizes far beyond these shapes and have no knob an existing test reaches them
with at 38 417 elements: they are left out."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import dropin_cases as D
from tests import workloads as W
from tests.containers import container, offsets

pytestmark = pytest.mark.gpu
EB = 1e-3
SENT = 7.5                                               # the sentinel element around a caller's array
BYTE = 0xA5                                              # ... and the byte around container bytes
SHAPES = {"flat": (64 * 600 + 17,), "2d": (150, 277), "3d": (22, 35, 53)}          # tests/test_container_layout_cpu.py's
FLAT_DIMS = (41, 937)                                    # 64 * 600 + 17 seen as a 2-D array by the flat box calls
CASES = [(m, k, d, t) for m in ("ec", "qt") for k in SHAPES for d in (np.float64, np.float32) for t in (False, True)]
IDS = [f"{m}-{k}-{np.dtype(d).name}-{'dzix' if t else 'zlib'}" for m, k, d, t in CASES]
T, SZ = C.POINTER(D.TVar), C.POINTER(C.c_size_t)


class DMissing(C.Structure):
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


def _lib(mode):
    lib = D._lib(mode)
    for name, args in (("dctz_decompress_range", [T, C.c_size_t, C.c_size_t, T]),
                       ("dctz_decompress_boxes", [T, C.c_int, SZ, C.c_int, SZ, SZ, C.POINTER(T)]),
                       ("dctz_decompress_box_nd", [T, SZ, SZ, T]),
                       ("dctz_decompress_boxes_nd", [T, C.c_int, SZ, SZ, C.POINTER(T)]),
                       ("dctz_decompress_coarse", [T, C.c_int, T]),
                       ("dctz_decompress_coarse_box_nd", [T, C.c_int, SZ, SZ, T]),
                       ("dctz_decompress_coarse_boxes_nd", [T, C.c_int, C.c_int, SZ, SZ, C.POINTER(T)]),
                       ("dctz_fixup_build", [T, T, C.c_int, C.c_double, C.POINTER(C.c_void_p), SZ]),
                       ("dctz_decompress_bounded", [T, C.c_void_p, C.c_size_t, T]),
                       ("dctz_compress_masked", [T, C.c_int, SZ, T, C.c_double, C.POINTER(DMissing), C.c_double, C.POINTER(C.c_void_p), SZ]),
                       ("dctz_decompress_masked", [T, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, T]),
                       ("dctz_compress_batch", [C.c_int, C.POINTER(T), C.POINTER(C.c_int), SZ, C.POINTER(T), C.POINTER(C.c_double)]),
                       ("dctz_decompress_batch", [C.c_int, C.POINTER(T), C.POINTER(T)])):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = args
    return lib


class Host:
    """A caller's array of n elements `shift` elements into a larger one filled with the sentinel (shift 0: at its start)."""

    def __init__(self, n, dtype, shift, init=None):
        self.all = np.full(n + 2, SENT, dtype)
        assert self.all.ctypes.data % 16 == 0
        self.a = self.all[shift:shift + n]
        if init is not None:
            self.a[:] = np.asarray(init).reshape(-1)
        if shift:
            assert self.a.ctypes.data % (2 * self.a.itemsize) == self.a.itemsize
        self.var = D._tvar(self.a)

    def intact(self):
        rest = np.ones(self.all.size, bool)
        off = (self.a.ctypes.data - self.all.ctypes.data) // self.a.itemsize
        rest[off:off + self.a.size] = False
        return bool((self.all[rest] == SENT).all())


class Bytes:
    """Container bytes (or room for them) `shift` bytes into a larger buffer of 0xA5."""

    def __init__(self, cap, dtype, shift, blob=None):
        self.all = np.full(cap + 32, BYTE, np.uint8)
        assert self.all.ctypes.data % 16 == 0
        self.shift, self.cap = shift, cap
        self.b = self.all[shift:shift + cap]
        if blob is not None:
            self.b[:len(blob)] = np.frombuffer(blob, np.uint8)
        self.var = D.TVar()
        self.var.datatype = 1 if np.dtype(dtype) == np.float64 else 0
        self.var.buf.d = C.cast(C.c_void_p(self.all.ctypes.data + shift), C.POINTER(C.c_double))

    def intact(self, used):
        return bool((self.all[:self.shift] == BYTE).all() and (self.all[self.shift + used:] == BYTE).all())


def _arr(v):
    return (C.c_size_t * len(v))(*[int(i) for i in v])


def _same(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.size == b.size and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_container(got, blob, c, dtype, qt, mean=True):
    """`got` against the oracle's container: the header fields, the streams (the sections are inflated: a zlib of another version
    deflates otherwise), the table and the extents.  Returns where `got` ends without a chunk index."""
    T_ = np.dtype(dtype)
    assert struct.unpack_from("<IIdI", got, 0) == struct.unpack_from("<IIdI", blob, 0), "datatype, N, error bound, count"
    assert got[24:24 + T_.itemsize] == blob[24:24 + T_.itemsize], "sf"
    if mean:                                             # (flat arrays: the serial-order mean, bit for bit)
        assert got[32:32 + T_.itemsize] == blob[32:32 + T_.itemsize], "mean"
    _, cnt, sizes, offs, end = D._sections(np.frombuffer(got, np.uint8), dtype, qt)
    assert cnt == c.cnt
    for off, size, want in zip(offs, sizes, (c.bin_index, c.dc, c.ac_exact)):
        assert zlib.decompress(got[off:off + size]) == want.tobytes()
    o = offsets(blob, qt)
    assert got[offs[2] + sizes[2]:end] == blob[o.get("table", o.get("nd", o.get("ix", o["end"]))):o.get("ix", o["end"])], "the table and the extents"
    return end


_made = {}


def _case(mode, kind, dtype, tail):
    """(x, the oracle's container, its streams, the oracle's decode), made once and never written."""
    key = (mode, kind, np.dtype(dtype).name, tail)
    if key not in _made:
        shape = SHAPES[kind]
        x = W.ragged(int(np.prod(shape)), dtype, scale=37.0).reshape(shape)
        m = O.QT if mode == "qt" else O.EC
        blob, c = container(x, EB, m, tail)
        full = O.decompress(c, O.FAST) if x.ndim == 1 else O.decompress_nd(c, x.shape, O.FAST)
        for a in (x, full):
            a.setflags(write=False)
        _made[key] = (x, blob, c, full)
    return _made[key]


@pytest.fixture()
def gpu_tail_env():
    yield
    os.environ.pop("DCTZ_ZLIB_GPU", None)


@pytest.mark.parametrize("mode,kind,dtype,tail", CASES, ids=IDS)
def test_compress_and_decompress_from_the_middle_of_larger_arrays(mode, kind, dtype, tail, gpu_tail_env):
    lib = _lib(mode)
    x, blob, c, full = _case(mode, kind, dtype, tail)
    n, qt = x.size, mode == "qt"
    xin = Host(n, dtype, 1, x)
    z = Bytes(n * x.itemsize + (1 << 16), dtype, 1)
    sz = C.c_size_t(0)
    if tail:
        os.environ["DCTZ_ZLIB_GPU"] = "1"
    if x.ndim > 1:
        assert lib.dctz_set_block_dims(x.ndim, _arr(x.shape)) == 0
    assert lib.dctz_compress(C.byref(xin.var), n, C.byref(sz), C.byref(z.var), EB) == 1
    os.environ.pop("DCTZ_ZLIB_GPU", None)
    got = bytes(z.b[:sz.value])
    assert xin.intact() and z.intact(sz.value), "dctz_compress wrote outside the caller's array or the container"
    # the container: the oracle's header fields and streams (the sections are inflated: a zlib of another version deflates otherwise)
    end = _check_container(got, blob, c, dtype, qt, mean=x.ndim == 1)
    assert (len(got) > end) == bool(tail) and (not tail or struct.unpack_from("<I", got, end)[0] == D.IX_MAGIC)
    if x.ndim == 1:
        assert _same(xin.a, c.scaled), "var->buf holds x / sf"
    # both containers, one byte in, decode to the oracle's array one element in
    for src in (got, blob):
        zz = Bytes(len(src), dtype, 1, src)
        r = Host(n, dtype, 1)
        assert lib.dctz_decompress(C.byref(zz.var), C.byref(r.var)) == 1
        assert _same(r.a, full) and r.intact() and _same(zz.b, np.frombuffer(src, np.uint8)) and zz.intact(len(src))


@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_batch_pair_from_the_middle_of_larger_arrays(mode):
    lib = _lib(mode)
    cases = [_case(mode, "flat", np.float64, False), _case(mode, "flat", np.float32, False)]
    k = len(cases)
    xs = [Host(x.size, x.dtype, 1, x) for x, _, _, _ in cases]
    zs = [Bytes(x.nbytes + (1 << 16), x.dtype, 1) for x, _, _, _ in cases]
    PT = T * k
    sizes = (C.c_size_t * k)()
    rc = lib.dctz_compress_batch(k, PT(*[C.pointer(h.var) for h in xs]), (C.c_int * k)(*[x.size for x, _, _, _ in cases]), sizes,
                                 PT(*[C.pointer(z.var) for z in zs]), (C.c_double * k)(*[EB] * k))
    assert rc == 1
    rs = [Host(x.size, x.dtype, 1) for x, _, _, _ in cases]
    assert lib.dctz_decompress_batch(k, PT(*[C.pointer(z.var) for z in zs]), PT(*[C.pointer(r.var) for r in rs])) == 1
    for (x, blob, c, full), h, z, r, size in zip(cases, xs, zs, rs, sizes):
        got = bytes(z.b[:size])
        assert _check_container(got, blob, c, x.dtype, mode == "qt") == len(got)
        assert _same(h.a, c.scaled) and h.intact() and z.intact(size)
        assert _same(r.a, full) and r.intact()


def _readers(lib, x, full, kind, mode):
    """[(name, call, expected or None)]: call(shift) runs one reader with its container `shift` bytes and its outputs `shift`
    elements into larger buffers and returns the outputs as a list of arrays (sentinels checked)."""
    n, dtype = x.size, x.dtype
    out = []

    def reader(name, want=None):
        def deco(f):
            out.append((name, f, want))
            return f
        return deco

    def outs(shift, sizes):
        return [Host(int(s), dtype, shift) for s in sizes]

    def done(rc, hosts, zz, blob):
        assert rc == 1 and all(h.intact() for h in hosts) and zz.intact(len(blob)) and _same(zz.b, np.frombuffer(blob, np.uint8))
        return [h.a.copy() for h in hosts]

    def ptrs(hosts):
        return (T * len(hosts))(*[C.pointer(h.var) for h in hosts])

    sl = lambda a, lo, hi: np.ascontiguousarray(a[tuple(slice(l, h) for l, h in zip(lo, hi))])      # noqa: E731
    ext = lambda lo, hi: int(np.prod([h - l for l, h in zip(lo, hi)]))                              # noqa: E731
    if kind == "flat":
        @reader("range", [full[5:n - 3]])
        def _(shift, zz, blob):
            h = outs(shift, [n - 8])
            return done(lib.dctz_decompress_range(C.byref(zz.var), 5, n - 3, C.byref(h[0].var)), h, zz, blob)
        view = full.reshape(FLAT_DIMS)
        boxes = [((3, 5), (40, 930)), ((0, 0), (1, 1)), ((17, 100), (18, 937))]

        @reader("box", [sl(view, *boxes[0])])
        def _(shift, zz, blob):
            lo, hi = boxes[0]
            h = outs(shift, [ext(lo, hi)])
            return done(lib.dctz_decompress_box(C.byref(zz.var), 2, _arr(FLAT_DIMS), _arr(lo), _arr(hi), C.byref(h[0].var)), h, zz, blob)

        @reader("boxes", [sl(view, lo, hi) for lo, hi in boxes])
        def _(shift, zz, blob):
            h = outs(shift, [ext(lo, hi) for lo, hi in boxes])
            lo, hi = [v for b in boxes for v in b[0]], [v for b in boxes for v in b[1]]
            return done(lib.dctz_decompress_boxes(C.byref(zz.var), 2, _arr(FLAT_DIMS), len(boxes), _arr(lo), _arr(hi), ptrs(h)), h, zz, blob)
        factors, cshape = (2, 64), lambda f: (-(-n // f),)                                          # noqa: E731
    else:
        shape = x.shape
        hi_ = tuple(v - 1 for v in shape)
        boxes = [(tuple(1 for _ in shape), hi_), (tuple(0 for _ in shape), tuple(1 for _ in shape)), (tuple(v // 2 for v in shape), shape)]

        @reader("box_nd", [sl(full, *boxes[0])])
        def _(shift, zz, blob):
            lo, hi = boxes[0]
            h = outs(shift, [ext(lo, hi)])
            return done(lib.dctz_decompress_box_nd(C.byref(zz.var), _arr(lo), _arr(hi), C.byref(h[0].var)), h, zz, blob)

        @reader("boxes_nd", [sl(full, lo, hi) for lo, hi in boxes])
        def _(shift, zz, blob):
            h = outs(shift, [ext(lo, hi) for lo, hi in boxes])
            lo, hi = [v for b in boxes for v in b[0]], [v for b in boxes for v in b[1]]
            return done(lib.dctz_decompress_boxes_nd(C.byref(zz.var), len(boxes), _arr(lo), _arr(hi), ptrs(h)), h, zz, blob)
        factors = (2, 8) if len(shape) == 2 else (2, 4)
        cshape = lambda f: tuple(-(-v // f) for v in shape)                                         # noqa: E731
        for f in factors:
            cs = cshape(f)
            cb = [(tuple(min(1, v - 1) for v in cs), cs), (tuple(0 for _ in cs), tuple(-(-v // 2) for v in cs))]

            @reader(f"coarse_box_nd/{f}")
            def _(shift, zz, blob, f=f, cb=cb):
                lo, hi = cb[0]
                h = outs(shift, [ext(lo, hi)])
                return done(lib.dctz_decompress_coarse_box_nd(C.byref(zz.var), f, _arr(lo), _arr(hi), C.byref(h[0].var)), h, zz, blob)

            @reader(f"coarse_boxes_nd/{f}")
            def _(shift, zz, blob, f=f, cb=cb):
                h = outs(shift, [ext(lo, hi) for lo, hi in cb])
                lo, hi = [v for b in cb for v in b[0]], [v for b in cb for v in b[1]]
                return done(lib.dctz_decompress_coarse_boxes_nd(C.byref(zz.var), f, len(cb), _arr(lo), _arr(hi), ptrs(h)), h, zz, blob)
    for f in factors:
        @reader(f"coarse/{f}")
        def _(shift, zz, blob, f=f):
            h = outs(shift, [int(np.prod(cshape(f)))])
            return done(lib.dctz_decompress_coarse(C.byref(zz.var), f, C.byref(h[0].var)), h, zz, blob)

    @reader("bounded")
    def _(shift, zz, blob):
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        ref = Host(n, dtype, shift, x)
        bound = 0.25 * float(np.abs(x.astype(np.float64) - full.astype(np.float64)).max())
        fix, nbytes = C.c_void_p(), C.c_size_t(0)
        assert lib.dctz_fixup_build(C.byref(zz.var), C.byref(ref.var), n, bound, C.byref(fix), C.byref(nbytes)) == 1
        try:
            assert _same(ref.a, x) and ref.intact()
            # (the blob is malloc's, 16-byte aligned: a copy one byte in is what a caller reads from a file)
            fb = np.full(nbytes.value + 2, BYTE, np.uint8)
            fb[1:1 + nbytes.value] = np.frombuffer(C.string_at(fix, nbytes.value), np.uint8)
            h = outs(shift, [n])
            res = done(lib.dctz_decompress_bounded(C.byref(zz.var), fb.ctypes.data + 1 if shift else fix, nbytes.value, C.byref(h[0].var)), h, zz, blob)
        finally:
            libc.free(fix)
        err = np.abs(x.reshape(-1).astype(np.float64) - res[0].astype(np.float64))
        assert float(err.max()) <= bound and int((res[0] != full.reshape(-1)).sum()) > 0, "the list corrects, and is not empty"
        return res
    return out


@pytest.mark.parametrize("mode,kind,dtype,tail", CASES, ids=IDS)
def test_partial_readers_from_the_middle_of_larger_arrays(mode, kind, dtype, tail):
    lib = _lib(mode)
    x, blob, c, full = _case(mode, kind, dtype, tail)
    ran = []
    for name, call, want in _readers(lib, x, full, kind, mode):
        base = call(0, Bytes(len(blob), dtype, 0, blob), blob)
        got = call(1, Bytes(len(blob), dtype, 1, blob), blob)
        assert len(got) == len(base) and all(_same(g, b) for g, b in zip(got, base)), f"{name}: the result moves with the placement"
        if want is not None:
            assert all(_same(g, w) for g, w in zip(got, want)), f"{name}: not the oracle's decode"
        ran.append(name.split("/")[0])
    flat = ["range", "box", "boxes", "coarse", "coarse", "bounded"]
    tiled = ["box_nd", "boxes_nd"] + ["coarse_box_nd", "coarse_boxes_nd"] * 2 + ["coarse", "coarse", "bounded"]
    assert ran == (flat if kind == "flat" else tiled)


@pytest.mark.parametrize("mode", ["ec", "qt"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_masked_pair_from_the_middle_of_larger_arrays(mode, dtype):
    """dctz_compress_masked / dctz_decompress_masked: the container and the mask are those of the call on buffers of their own."""
    lib = _lib(mode)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    n = SHAPES["flat"][0]
    x = W.ragged(n, dtype, scale=37.0)
    miss = np.zeros(n, bool)
    miss[np.random.default_rng(3).random(n) < 0.05] = True
    miss[64:128] = True
    miss[-1] = True
    x[miss] = 1e36
    rule = DMissing(4, 1e36, 0.0)                         # DCTZ_MISS_VALUE
    res = []
    for shift in (0, 1):
        xin = Host(n, dtype, shift, x)
        z = Bytes(n * x.itemsize + (1 << 16), dtype, shift)
        sz, blob, nbytes = C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
        assert lib.dctz_compress_masked(C.byref(xin.var), n, C.byref(sz), C.byref(z.var), EB, C.byref(rule), -1.0, C.byref(blob), C.byref(nbytes)) == 1
        try:
            assert xin.intact() and z.intact(sz.value)
            mb = np.full(nbytes.value + 2, BYTE, np.uint8)
            mb[shift:shift + nbytes.value] = np.frombuffer(C.string_at(blob, nbytes.value), np.uint8)
            r = Host(n, dtype, shift)
            assert lib.dctz_decompress_masked(C.byref(z.var), mb.ctypes.data + shift, nbytes.value, None, 0, C.byref(r.var)) == 1
            assert r.intact() and bool((r.a[miss] == dtype(-1.0)).all()) and bool((np.abs(r.a[~miss]) < 1e3).all())
            res.append((bytes(z.b[:sz.value]), C.string_at(blob, nbytes.value), r.a.copy(), xin.a.copy()))
        finally:
            libc.free(blob)
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and _same(res[0][2], res[1][2]) and _same(res[0][3], res[1][3])
