"""CPU-side checks of the remembered sf guess: dctzhip_set_spec_memory is exported by libdctzhip.so, declared in the header
and bound in Python; the two counters are documented; a NULL context is refused before a GPU is touched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dctz_amd", "lib")
E_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(os.path.join(LIB, "libdctzhip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dctz_amd"), "all"])


def test_shim_exports_the_setter():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIB, "libdctzhip.so")], text=True)
    assert "dctzhip_set_spec_memory" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    import dctz_amd
    from dctz_amd import hip as H
    assert hasattr(dctz_amd.load_library(), "dctzhip_set_spec_memory") and hasattr(H.Context, "set_spec_memory")


def test_header_declares_the_setter_and_the_counters():
    text = open(os.path.join(ROOT, "include", "dctz_hip.h")).read()
    assert re.search(r"int\s+dctzhip_set_spec_memory\s*\(\s*dctzhip_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    assert "DCTZHIP_SPEC_MEMORY" in text
    counters = text[text.index("Counters of the context"):text.index("int dctzhip_debug_counter")]
    assert "18 / 19" in counters


def test_prototype_compiles_as_c(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "dctz_hip.h"\nint (*p)(dctzhip_ctx *, int) = dctzhip_set_spec_memory;\n')
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"), str(src)])


def test_null_context_is_refused():
    import dctz_amd
    lib = dctz_amd.load_library()
    assert lib.dctzhip_set_spec_memory(None, 1) == E_ARG
