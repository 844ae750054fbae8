"""CPU check of the host structure of a position problem (csrc/pos_structure.hpp): the host compiler builds
tests/cpp/pos_structure_test.cpp against the header -- the CSR of the directed entries of a 5-camera, 6-edge graph with an isolated camera, a
repeated pair and a pair in both orientations as literals, and a 200-camera, 1500-edge random graph against a plain sort."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_build(tmp_path):
    exe = str(tmp_path / "pos_structure_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pos_structure_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
