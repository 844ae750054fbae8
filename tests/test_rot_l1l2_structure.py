"""CPU check of the host structure of the robust L1 + IRLS rotation estimator (csrc/rot_l1l2_structure.hpp): the host compiler builds
tests/cpp/rot_l1l2_structure_test.cpp against the header -- a 5-camera graph with a repeated pair, a pair in both orientations and an
isolated camera as literals, a hub with the fixed camera at the hub and at a leaf, rows on either side of the lane-class threshold, a
random multigraph against the edge list, and the connectivity check."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_build(tmp_path):
    exe = str(tmp_path / "rot_l1l2_structure_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rot_l1l2_structure_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
