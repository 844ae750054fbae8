"""CPU check of the slab layout of the one-shot device calls (csrc/flat_call.hpp): the host compiler builds tests/cpp/flat_layout_test.cpp
against the header -- 256-byte offsets in take order, no overlap, nothing for a zero count, the total, and the offsets of the translation
refinement's arrays for E = 3, N = 2, M = 5 as literals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_arithmetic(tmp_path):
    exe = str(tmp_path / "flat_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "flat_layout_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
