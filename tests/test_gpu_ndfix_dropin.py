"""The drop-in path of the correction list for DZND containers (include/dctz.h: dctz_fixup_build, dctz_decompress_bounded; the
container decides): dctz_set_block_dims + dctz_compress -> dctz_fixup_build -> the version-2 blob -> dctz_decompress_bounded.
The result meets the guarantee and equals dctz_decompress wherever nothing was listed; a shortened blob, a blob with an offset
on a padded position and a flat blob return -1 and leave the output untouched."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import dropin_cases as D
from tests import ndfix_cases as N

pytestmark = pytest.mark.gpu

SHAPES = [(45, 77), (13, 22, 35)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", ["ec", "qt"])
def test_dropin_round_trip(mode, dtype, shape):
    lib = D._lib(mode)
    lib.dctz_fixup_build.restype = C.c_int
    lib.dctz_fixup_build.argtypes = [C.POINTER(D.TVar), C.POINTER(D.TVar), C.c_int, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.dctz_decompress_bounded.restype = C.c_int
    lib.dctz_decompress_bounded.argtypes = [C.POINTER(D.TVar), C.c_void_p, C.c_size_t, C.POINTER(D.TVar)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    x = N.field(shape, "noisy", dtype)
    n = x.size
    es = np.dtype(dtype).itemsize
    flat = x.reshape(-1)
    assert lib.dctz_set_block_dims(len(shape), (C.c_size_t * len(shape))(*shape)) == 0
    try:
        z, full = D._container(lib, flat, N.EB, False)
    finally:
        assert lib.dctz_set_block_dims(0, None) == 0
    zflat, _ = D._container(lib, flat, N.EB, False)                 # the same array in flat blocks
    full = full.reshape(shape)
    zv = D._tvar(z.view(dtype)[: z.size // es])
    zfv = D._tvar(zflat.view(dtype)[: zflat.size // es])
    bound = 0.5 * N.EB * 100.0
    lm, ws, wo, wv = N.fix_list(x, full, bound)
    k = int(ws[-1])
    assert 100 < k < n
    blob, nbytes = C.c_void_p(), C.c_size_t(0)
    fblob, fbytes = C.c_void_p(), C.c_size_t(0)
    ref = flat.copy()
    assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n, bound, C.byref(blob), C.byref(nbytes)) == 1
    assert lib.dctz_fixup_build(C.byref(zfv), C.byref(D._tvar(ref)), n, bound, C.byref(fblob), C.byref(fbytes)) == 1
    try:
        raw = C.string_at(blob, nbytes.value)
        tiles = N.tiles(shape)
        # the version-2 header: the 48 bytes of version 1 with ndims in the zero field, then the extents
        assert raw[:4] == b"DZFX"
        ver, dt, nd = struct.unpack_from("<III", raw, 4)
        hn, ht, hc = struct.unpack_from("<QQQ", raw, 16)
        hb, = struct.unpack_from("<d", raw, 40)
        hd = struct.unpack_from("<QQQ", raw, 48)
        assert (ver, dt, nd) == (2, 1 if dtype == np.float64 else 0, len(shape))
        assert (hn, ht, hc, hb) == (n, tiles, k, bound) and list(hd) == (list(shape) + [0])[:3]
        pad8 = lambda v: (v + 7) & ~7
        off_at = 72 + pad8(4 * (tiles + 1))
        val_at = off_at + pad8(2 * k)
        assert len(raw) == val_at + k * es
        assert np.array_equal(np.frombuffer(raw, np.uint32, tiles + 1, 72), ws)
        assert np.array_equal(np.frombuffer(raw, np.uint16, k, off_at), wo)
        assert np.array_equal(_bits(np.frombuffer(raw, dtype, k, val_at)), _bits(wv))
        assert not any(raw[72 + 4 * (tiles + 1):off_at]) and not any(raw[off_at + 2 * k:val_at])
        # the flat blob of the flat container is version 1, 48 bytes of header, as it always was
        fraw = C.string_at(fblob, fbytes.value)
        assert struct.unpack_from("<III", fraw, 4) == (1, dt, 0) and struct.unpack_from("<Q", fraw, 16)[0] == n

        out = np.full(n, -7.25e11, dtype)
        assert lib.dctz_decompress_bounded(C.byref(zv), blob, nbytes.value, C.byref(D._tvar(out))) == 1
        got = out.reshape(shape)
        assert np.array_equal(_bits(got), _bits(np.where(lm, x, full)))
        assert N.guarantee_holds(x, got, bound)
        assert np.array_equal(_bits(got[~lm]), _bits(full[~lm]))

        def refused(b, nb, zvar=zv):
            o = np.full(n, -7.25e11, dtype)
            keep = o.copy()
            assert lib.dctz_decompress_bounded(C.byref(zvar), b, nb, C.byref(D._tvar(o))) == -1
            assert np.array_equal(_bits(o), _bits(keep))

        refused(blob, nbytes.value - 8)                                         # shortened
        refused(fblob, fbytes.value)                                            # a flat blob with the tiled container
        refused(blob, nbytes.value, zfv)                                        # ... and the tiled blob with the flat container
        # one offset moved onto a padded position, ascending order kept: the apply kernel's own check
        pad = ~N.real(shape)
        tam = None
        for t in range(tiles):
            for i in range(int(ws[t]), int(ws[t + 1])):
                lo = int(wo[i - 1]) + 1 if i > int(ws[t]) else 0
                cand = [o for o in range(lo, int(wo[i])) if pad[t * N.TILE + o]]
                if cand:
                    tam = bytearray(raw)
                    struct.pack_into("<H", tam, off_at + 2 * i, cand[0])
                    break
            if tam:
                break
        assert tam is not None
        tb = (C.c_char * len(tam)).from_buffer(tam)
        refused(tb, len(tam))
        # the good blob still works afterwards
        assert lib.dctz_decompress_bounded(C.byref(zv), blob, nbytes.value, C.byref(D._tvar(out))) == 1
        assert np.array_equal(_bits(out.reshape(shape)), _bits(np.where(lm, x, full)))
    finally:
        libc.free(blob)
        libc.free(fblob)
    again = np.empty(n, dtype)
    assert lib.dctz_decompress(C.byref(zv), C.byref(D._tvar(again))) == 1
    assert np.array_equal(_bits(again.reshape(shape)), _bits(full))
    # refusals of the build: a reference of another length (the stream positions are not the length) or type, a bad bound
    nb = C.c_size_t(0)
    bl = C.c_void_p()
    assert 64 * N.nblk(shape) != n
    assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(np.zeros(64 * N.nblk(shape), dtype))), 64 * N.nblk(shape), bound, C.byref(bl), C.byref(nb)) == -1
    assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n - 1, bound, C.byref(bl), C.byref(nb)) == -1
    other = ref.astype(np.float32 if dtype == np.float64 else np.float64)
    assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(other)), n, bound, C.byref(bl), C.byref(nb)) == -1
    assert lib.dctz_fixup_build(C.byref(zv), C.byref(D._tvar(ref)), n, -1.0, C.byref(bl), C.byref(nb)) == -1
