"""Placement of the container bytes on the host ("Placement, what is pinned"): dctz_check_container,
shallow and deep, returns the same code for a container that starts 1 ... 7 bytes past a 16-byte boundary as for one that
starts on it -- for every kind and every damage of the fixed list of tests/test_container_layout_cpu.py.  An HPC caller hands
over a record out of the middle of a larger buffer; the header's fields are then at odd addresses.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import test_container_layout_cpu as L


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(L.DUMP):
        import __graft_entry__ as g
        g.build()
    fns = {}
    for mode, name in ((L.O.EC, "ec"), (L.O.QT, "qt")):
        lib = C.CDLL(os.path.join(L.LIBDIR, f"libdctz-{name}.so"))       # (a handle of its own: the argtypes below are this file's)
        fns[mode] = lib["dctz_check_container"]
        fns[mode].restype = C.c_int
        fns[mode].argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    return fns


def _at(blob, off):
    """(the holder, the address) of a copy of `blob` that starts `off` bytes past a 16-byte boundary, 0xA5 around it."""
    buf = np.full(len(blob) + 64, 0xA5, np.uint8)
    start = (-buf.ctypes.data) % 16 + 16 + off
    buf[start:start + len(blob)] = np.frombuffer(blob, np.uint8)
    assert (buf.ctypes.data + start) % 16 == off
    return buf, buf.ctypes.data + start


@pytest.mark.parametrize("kind,dtype,indexed", L.CASES, ids=L.IDS)
def test_check_container_does_not_depend_on_where_the_bytes_start(check, kind, dtype, indexed):
    x, mode, blob, c = L.make(kind, dtype, indexed)
    f = check[mode]
    cases = [("sound", blob)] + L.damages(blob, mode, x.ndim if x.ndim > 1 else 0, indexed)
    for name, b in cases:
        codes = []
        for off in range(8):
            buf, p = _at(b, off)
            codes.append((f(p, len(b), 0, 0), f(p, len(b), 0, 1)))
            assert int((buf != 0xA5).sum()) <= len(b) and buf[:16].tolist() == [0xA5] * 16, "the check writes nothing"
        assert codes == [codes[0]] * 8, (name, codes)
        want = (L.OK, L.OK) if name == "sound" else L.EXPECT_KIND.get((kind, indexed, name), L.EXPECT.get(name))
        assert codes[0] == want, (name, codes[0], want)
