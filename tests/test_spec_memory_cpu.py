"""The policy of dctz_amd/csrc/dctz_spec_memory.h, driven on the CPU by tests/c/spec_memory_test.cpp: built as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_under_sanitizers(tmp_path):
    exe = str(tmp_path / "spec_memory_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dctz_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "spec_memory_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("spec memory ok")
