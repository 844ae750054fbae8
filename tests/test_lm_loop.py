"""CPU check of the host control loops of the position and bundle solvers (csrc/lm_loop.hpp: lm_loop and pcg_loop, used by solver_pos.hpp,
solver_ba.hpp and solver_full_ba.hpp): the host compiler alone builds tests/cpp/lm_loop_test.cpp against the header, which is part of the check.
The program drives the Levenberg-Marquardt loop with scripted operations (every ending, five invalid steps, the radii against
trust_region.hpp bit for bit, statuses) and the PCG driver with scripted r.M^-1 r sequences under both settings of its breakdown flag."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scripted_lm_and_pcg_loops(tmp_path):
    exe = str(tmp_path / "lm_loop_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lm_loop_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
