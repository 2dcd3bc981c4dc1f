"""Helpers shared by the host-only container tests: `.z` files assembled from the oracle's streams, and the host twin of
the device entropy stage (tests/emu/emu_deflate.cpp) that makes 78 5E chunked streams and their per-chunk size lists.

Layout (include/dctz.h):  header | bin_index.z | DC.z | AC_exact.z | [qtable] | ["DZND" + extents] | ["DZIX" chunk index]"""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 128 * 128
ND_MAGIC, IX_MAGIC = 0x444E5A44, 0x58495A44


def twin():
    so = os.path.join(ROOT, "tests", "emu", "emu_deflate.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_deflate.cpp")
    hdr = os.path.join(ROOT, "dctz_amd", "csrc", "deflate_chunk.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dctz_amd", "csrc"), src, "-o", so], check=True)
    L = C.CDLL(so)
    L.emu_deflate.restype = C.c_size_t
    L.emu_deflate.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    L.emu_deflate_index.restype = C.c_size_t
    L.emu_deflate_index.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.emu_deflate_literals.restype = C.c_size_t
    L.emu_deflate_literals.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.emu_deflate_bound.restype = C.c_size_t
    L.emu_deflate_bound.argtypes = [C.c_size_t, C.c_int]
    return L


def twin_deflate(L, data, nthr=128, want_index=False, literals=False):
    a = np.frombuffer(data, dtype=np.uint8)
    cap = L.emu_deflate_bound(len(data), nthr)
    out = np.zeros(cap, dtype=np.uint8)
    chunk = nthr * 128
    sizes = np.zeros(max(1, (len(data) + chunk - 1) // chunk), np.uint32)
    n = (L.emu_deflate_literals if literals else L.emu_deflate_index)(a.ctypes.data if len(data) else None, len(data), out.ctypes.data, cap, nthr,
                                                                     sizes.ctypes.data)
    assert n > 0
    if want_index:
        return out[:n].tobytes(), sizes[:(len(data) + chunk - 1) // chunk]
    return out[:n].tobytes()


def container(x, eb, mode, indexed=False):
    """A .z file assembled from the oracle's streams (dctz-comp-lib.c:775-820).  x.ndim 2 / 3: multi-dimensional blocks --
    the geometry in bits 8..15 of `datatype`, "DZND" + three extents behind the last section (the table, in QT).
    indexed: the sections as the device entropy stage writes them (host twin, DC and AC_exact as literals like the drop-in)
    and the "DZIX" chunk index behind everything else.  Returns (bytes, the oracle's result)."""
    nd = x.ndim if x.ndim > 1 else 0
    c = O.compress_nd(x, eb, mode, O.FAST) if nd else O.compress(x, eb, mode, O.FAST)
    raw = [c.bin_index.tobytes(), c.dc.tobytes(), c.ac_exact.tobytes()]
    if indexed:
        L = twin()
        zi = [twin_deflate(L, b, want_index=True, literals=i > 0) for i, b in enumerate(raw)]
        z, sizes = [p[0] for p in zi], [p[1] for p in zi]
    else:
        z = [zlib.compress(b) for b in raw]
    is_d = x.dtype == np.float64
    h = bytearray(56)
    struct.pack_into("<II", h, 0, (1 if is_d else 0) | (nd << 8), x.size)
    struct.pack_into("<d", h, 8, eb)
    struct.pack_into("<I", h, 16, c.cnt)
    struct.pack_into("<d" if is_d else "<f", h, 24, c.sf)
    struct.pack_into("<d" if is_d else "<f", h, 32, c.mean)
    struct.pack_into("<III", h, 40, len(z[0]), len(z[1]), len(z[2]))
    if mode == O.QT:
        struct.pack_into("<I", h, 52, c.bin_index.size)
    blob = bytes(h) + b"".join(z)
    if mode == O.QT:
        blob += c.qtable.tobytes()
    if nd:
        blob += struct.pack("<IIII", ND_MAGIC, *(list(x.shape) + [0] * (3 - nd)))
    if indexed:
        ix = struct.pack("<IIIII", IX_MAGIC, CHUNK, *(len(s) for s in sizes)) + b"".join(s.astype("<u2").tobytes() for s in sizes)
        blob += ix + b"\0" * (-len(ix) % 4)
    return blob, c


def offsets(blob, qt):
    """Where the parts of a container made by container() begin: a dict of byte offsets, in layout order ("end": the
    container's size; "ix_entries" / "ix_pad": the chunk sizes / the padding behind them)."""
    dt, n = struct.unpack_from("<II", blob, 0)
    z = struct.unpack_from("<III", blob, 40)
    o = {"sec0": 56, "sec1": 56 + z[0], "sec2": 56 + z[0] + z[1]}
    cur = 56 + sum(z)
    if qt:
        o["table"] = cur
        cur += 64 * (8 if dt & 0xff else 4)
    if (dt >> 8) & 0xff:
        o["nd"] = cur
        cur += 16
    if cur < len(blob):
        counts = struct.unpack_from("<III", blob, cur + 8)
        o["ix"], o["ix_entries"], o["ix_pad"] = cur, cur + 20, cur + 20 + 2 * sum(counts)
    o["end"] = len(blob)
    return o
