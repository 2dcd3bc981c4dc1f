"""One hot kernel per translation unit (dctz_kernels.hip): the part objects the Makefile builds hold one kernel
each, together exactly the flat k_compress forms and the k_compress_batch forms, and no kernel of the library sits in two
code objects (read from the code objects' metadata)."""
import glob
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dctz_amd", "lib")
LIB = os.path.join(LIBDIR, "libdctzhip.so")
PARTS = sorted(glob.glob(os.path.join(LIBDIR, "dctz_kernels_p*.o")))

TYPES, MODES, FLAGS = ("double", "float"), (0, 1), ("false", "true")
PH_C = 2            # Phases<T>::C of both element types (dctz_device.h: DCTZ_PHC64, DCTZ_PHC32)
GEOM_1D = 0
# the 16 flat forms (type x mode x STATS x SC) and the 8 batch forms (type x mode x STATS)
HOT = {f"dctz::k_compress<{t}, {m}, {st}, {PH_C}, {GEOM_1D}, {sc}>" for t, m, st, sc in itertools.product(TYPES, MODES, FLAGS, FLAGS)} | \
      {f"dctz::k_compress_batch<{t}, {m}, {st}>" for t, m, st in itertools.product(TYPES, MODES, FLAGS)}


def _names(path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels_of
    return [k["demangled"].split("(")[0] for k in kernels_of(path)]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdctzhip.so is not built")
def test_no_kernel_in_two_code_objects():
    names = _names(LIB)
    twice = sorted({n for n in names if names.count(n) > 1})
    assert not twice, twice
    assert HOT <= set(names), sorted(HOT - set(names))


@pytest.mark.skipif(not os.path.exists(LIB) or not PARTS, reason="libdctzhip.so and its part objects are not built")
def test_part_objects_are_the_hot_kernels():
    assert len(HOT) == 24
    per = {os.path.basename(p): _names(p) for p in PARTS}
    for obj, names in per.items():
        assert len(names) == 1, (obj, names)
    assert {n[0] for n in per.values()} == HOT
    assert len(PARTS) == len(HOT)
