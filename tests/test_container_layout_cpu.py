"""The .z container layout, pinned on the host (include/dctz.h):

    header | bin_index.z | DC.z | AC_exact.z | [qtable] | ["DZND" + extents] | ["DZIX" chunk index]

Characterisation of the two entry points that read a container without a GPU -- dctz_check_container (shallow and deep)
and `dctz-dump [-v]` -- on containers assembled from the oracle's streams: fp32 / fp64 x {flat EC, flat QT, 2-D, 3-D} x
{plain zlib sections, chunked sections + "DZIX"}.  The return codes below are what the library returned when this file was
written (recorded by running it, not reasoned out); the surprising ones carry a comment.  Every reader and writer of the
drop-in library shares this layout, so a change here is a change of the format."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import workloads as W
from tests.containers import CHUNK, container, offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dctz_amd", "lib")
DUMP = os.path.join(ROOT, "dctz_amd", "bin", "dctz-dump")
OK, TRUNCATED, BAD_HEADER, TOO_LARGE, BAD_STREAM = 0, -1, -2, -3, -4

# a short last block / edge tiles, and more than one chunk of bin_index (16 KiB each)
KINDS = {"flat_ec": (O.EC, (64 * 600 + 17,)), "flat_qt": (O.QT, (64 * 600 + 17,)), "2d": (O.EC, (150, 277)), "3d": (O.QT, (22, 35, 53))}
CASES = [(kind, dtype, indexed) for kind in KINDS for dtype in (np.float64, np.float32) for indexed in (False, True)]
IDS = [f"{k}-{np.dtype(d).name}-{'dzix' if i else 'zlib'}" for k, d, i in CASES]


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(DUMP):
        import __graft_entry__ as g
        g.build()
    out = {}
    for mode, name in ((O.EC, "ec"), (O.QT, "qt")):
        out[mode] = C.CDLL(os.path.join(LIBDIR, f"libdctz-{name}.so"))
        out[mode].dctz_check_container.restype = C.c_int
        out[mode].dctz_check_container.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
    return out


_made = {}


def make(kind, dtype, indexed):
    key = (kind, np.dtype(dtype).name, indexed)
    if key not in _made:
        mode, shape = KINDS[kind]
        x = W.ragged(int(np.prod(shape)), dtype, scale=37.0).reshape(shape)
        blob, c = container(x, 1e-3, mode, indexed)
        _made[key] = (x, mode, blob, c)
    return _made[key]


def _put(blob, fmt, off, *v):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, *v)
    return bytes(b)


def damages(blob, mode, nd, indexed):
    """The fixed list: (name, bytes).  "cut:<part>": the container one byte short of the END of that part."""
    o = offsets(blob, mode == O.QT)
    dt, n = struct.unpack_from("<II", blob, 0)
    ends = [("header", 56), ("sec0", o["sec1"]), ("sec1", o["sec2"]), ("sec2", o.get("table", o.get("nd", o.get("ix", o["end"]))))]
    if "table" in o:
        ends.append(("table", o.get("nd", o.get("ix", o["end"]))))
    if "nd" in o:
        ends.append(("nd", o["nd"] + 16))
    if "ix" in o:
        ends += [("ix_header", o["ix_entries"]), ("ix_entries", o["ix_pad"])]
    ends.append(("end", o["end"]))
    out = [(f"cut:{name}", blob[:e - 1]) for name, e in ends]
    out.append(("datatype_high_bits", _put(blob, "<I", 0, dt | (1 << 16))))
    out.append(("geometry_1", _put(blob, "<I", 0, (dt & 0xff) | (1 << 8))))
    out.append(("geometry_4", _put(blob, "<I", 0, (dt & 0xff) | (4 << 8))))
    out.append(("eb_nan", _put(blob, "<d", 8, float("nan"))))
    if mode == O.QT:
        out.append(("bindex_count+1", _put(blob, "<I", 52, struct.unpack_from("<I", blob, 52)[0] + 1)))
    if nd:
        d = struct.unpack_from("<III", blob, o["nd"] + 4)
        out.append(("dznd_magic", _put(blob, "<I", o["nd"], 0x444E5A45)))
        out.append(("extents_product", _put(blob, "<I", o["nd"] + 4, d[0] + 1)))
        if nd == 2:
            out.append(("2d_third_extent", _put(blob, "<I", o["nd"] + 12, 1)))
    if indexed:
        n0 = struct.unpack_from("<I", blob, o["ix"] + 8)[0]
        e0 = struct.unpack_from("<H", blob, o["ix_entries"])[0]
        out.append(("dzix_magic", _put(blob, "<I", o["ix"], 0x58495A45)))
        out.append(("chunk_1023", _put(blob, "<I", o["ix"] + 4, 1023)))
        out.append(("chunk_65536", _put(blob, "<I", o["ix"] + 4, 65536)))
        out.append(("count+1", _put(blob, "<I", o["ix"] + 8, n0 + 1)))
        out.append(("size+1", _put(blob, "<H", o["ix_entries"], e0 + 1)))
        out.append(("no_trailer", blob[:o["ix"]]))
    return out


# name -> (shallow, deep).  Recorded from the library.
EXPECT = {
    "cut:header": (TRUNCATED, TRUNCATED), "cut:sec0": (TRUNCATED, TRUNCATED), "cut:sec1": (TRUNCATED, TRUNCATED),
    "cut:sec2": (TRUNCATED, TRUNCATED), "cut:table": (TRUNCATED, TRUNCATED), "cut:nd": (TRUNCATED, TRUNCATED),
    "cut:ix_header": (TRUNCATED, TRUNCATED), "cut:ix_entries": (TRUNCATED, TRUNCATED), "cut:end": (TRUNCATED, TRUNCATED),
    "datatype_high_bits": (BAD_HEADER, BAD_HEADER), "geometry_1": (BAD_HEADER, BAD_HEADER), "geometry_4": (BAD_HEADER, BAD_HEADER),
    "eb_nan": (BAD_HEADER, BAD_HEADER), "bindex_count+1": (BAD_HEADER, BAD_HEADER),
    "dznd_magic": (BAD_HEADER, BAD_HEADER), "extents_product": (BAD_HEADER, BAD_HEADER), "2d_third_extent": (BAD_HEADER, BAD_HEADER),
    # a marked container (78 5E sections) whose index is wrong is a bad STREAM, not a bad header; without any trailer it is truncated
    "dzix_magic": (BAD_STREAM, BAD_STREAM), "chunk_1023": (BAD_STREAM, BAD_STREAM), "chunk_65536": (BAD_STREAM, BAD_STREAM),
    "count+1": (BAD_STREAM, BAD_STREAM), "size+1": (BAD_STREAM, BAD_STREAM), "no_trailer": (TRUNCATED, TRUNCATED),
}
# (kind, indexed, name) -> (shallow, deep) where a container kind differs from the table above
# Surprising, kept: the check asks for the index's 20 bytes + 2 per chunk, not for the padding to a multiple of 4 behind them.
# These containers have an odd number of chunks, so one byte short of the end is still accepted ("3d" has an even number:
# its end is the end of the entries).
EXPECT_KIND = {
    ("flat_ec", True, "cut:end"): (OK, OK), ("flat_qt", True, "cut:end"): (OK, OK), ("2d", True, "cut:end"): (OK, OK),
}


@pytest.mark.parametrize("kind,dtype,indexed", CASES, ids=IDS)
def test_check_container_codes(libs, kind, dtype, indexed):
    x, mode, blob, c = make(kind, dtype, indexed)
    lib = libs[mode]
    chk = lambda b, deep: lib.dctz_check_container(bytes(b), len(b), 0, deep)
    for deep in (0, 1):
        assert chk(blob, deep) == OK
        assert chk(blob + b"\0" * 7, deep) == OK                      # slack bytes behind the container
        assert lib.dctz_check_container(blob, len(blob), x.size, deep) == OK
    got = {name: (chk(b, 0), chk(b, 1)) for name, b in damages(blob, mode, x.ndim if x.ndim > 1 else 0, indexed)}
    want = {name: EXPECT_KIND.get((kind, indexed, name), EXPECT.get(name)) for name in got}
    assert got == want


def dump_lines(path, x, mode, blob, c, verbose):
    """What dctz-dump prints for a sound container made by container() (dctz_amd/cli/dctz_dump.c)."""
    is_d = x.dtype == np.float64
    ts = 8 if is_d else 4
    out = [f"File Name={path}", f"data type={'double' if is_d else 'float'}", f"N={x.size}", "error_bound=0.001000",
           f"total # of AC_exact={c.cnt}", f"SF={float(c.sf):f}"]
    if not verbose:
        return out
    qt = mode == O.QT
    o = offsets(blob, qt)
    z = struct.unpack_from("<III", blob, 40)
    nblk, npos = c.dc.size, c.bin_index.size
    if x.ndim == 2:
        out.append(f"multi-dimensional blocks: {x.shape[0]} x {x.shape[1]} array, 8 x 8 tiles")
    if x.ndim == 3:
        out.append(f"multi-dimensional blocks: {x.shape[0]} x {x.shape[1]} x {x.shape[2]} array, 4 x 4 x 4 tiles")
    out.append(f"mean={float(np.frombuffer(blob[32:32 + ts], x.dtype)[0]):.17g}")
    out.append(f"blocks={nblk} (last one {x.size % 64 if x.ndim == 1 and x.size % 64 else 64} elements)")
    out.append(f"bin_index: offset {o['sec0']}, {z[0]} bytes deflated ({npos} raw)")
    out.append(f"DC:        offset {o['sec1']}, {z[1]} bytes deflated ({nblk * 4} raw)")
    out.append(f"AC_exact:  offset {o['sec2']}, {z[2]} bytes deflated ({c.cnt * 4} raw)")
    fsz = o.get("ix", o["end"])
    if qt:
        out.append(f"variant=qt, bindex_count={npos}, table at offset {o['table']}, file size {fsz} = layout")
        out.append("qtable[1..4]=" + ", ".join(f"{float(v):.9g}" for v in c.qtable[1:5]))
    else:
        out.append(f"variant=ec (no table), file size {fsz} = layout")
    if "ix" in o:
        n = struct.unpack_from("<III", blob, o["ix"] + 8)
        out.append(f"chunk index: {o['end'] - o['ix']} bytes at offset {o['ix']}, chunks of {CHUNK} bytes: {n[0]} + {n[1]} + {n[2]} "
                   "(sections made by the GPU entropy stage)")
        out.append("chunk index tiles the three streams")
    out.append(f"compression ratio={x.nbytes / len(blob):.2f}")
    return out


def _dump(path, verbose):
    r = subprocess.run([DUMP] + (["-v"] if verbose else []) + [str(path)], capture_output=True, text=True)
    return r.returncode, r.stdout.splitlines()


@pytest.mark.parametrize("kind,dtype,indexed", CASES, ids=IDS)
def test_dump_output_line_for_line(libs, tmp_path, kind, dtype, indexed):
    x, mode, blob, c = make(kind, dtype, indexed)
    f = tmp_path / "a.z"
    f.write_bytes(blob)
    for verbose in (False, True):
        assert _dump(f, verbose) == (0, dump_lines(f, x, mode, blob, c, verbose))


def test_dump_reports_damage(libs, tmp_path):
    """One case each of: an index that does not tile, a file size no variant explains, geometry without extents."""
    f = tmp_path / "bad.z"
    # a chunk size off by one: the index is found (magic, total size) but its sizes no longer add up to the section's
    x, mode, blob, c = make("flat_qt", np.float64, True)
    o = offsets(blob, True)
    e0 = struct.unpack_from("<H", blob, o["ix_entries"])[0]
    f.write_bytes(_put(blob, "<H", o["ix_entries"], e0 + 1))
    good = dump_lines(f, x, mode, blob, c, True)
    assert _dump(f, True) == (2, good[:-2] + ["chunk index does NOT tile the streams", good[-1]])
    # five bytes cut off a plain container: neither the ec nor the qt layout
    x, mode, blob, c = make("flat_ec", np.float32, False)
    f.write_bytes(blob[:-5])
    good = dump_lines(f, x, mode, blob, c, True)
    assert _dump(f, True) == (2, good[:-2] + [f"LAYOUT MISMATCH: header describes {len(blob)} bytes (ec) or {len(blob) + 256} (qt), file has {len(blob) - 5}",
                                             f"compression ratio={x.nbytes / (len(blob) - 5):.2f}"])
    # "DZND" damaged: the header says 2-D, the end of the file does not
    x, mode, blob, c = make("2d", np.float64, False)
    o = offsets(blob, False)
    f.write_bytes(_put(blob, "<I", o["nd"], 0x444E5A45))
    good = dump_lines(f, x, mode, blob, c, True)
    nblk_flat = (x.size + 63) // 64
    want = good[:6] + ["LAYOUT MISMATCH: geometry 2 in the header but no extents at the end of the file", good[7],
                       f"blocks={nblk_flat} (last one 64 elements)", good[9].replace(f"({c.bin_index.size} raw)", f"({x.size} raw)"),
                       good[10].replace(f"({c.dc.size * 4} raw)", f"({nblk_flat * 4} raw)")] + good[11:]
    assert _dump(f, True) == (2, want)
