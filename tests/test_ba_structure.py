"""CPU check of the host structure of a bundle-adjustment problem (csrc/ba_structure.hpp): the host compiler builds
tests/cpp/ba_structure_test.cpp against the header -- used observations, active sets and the per-camera CSR of a hand-made case with an
unestimated camera and track as literals, the empty cases, and 2000 random tracks against a plain stable sort."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_build(tmp_path):
    exe = str(tmp_path / "ba_structure_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ba_structure_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
