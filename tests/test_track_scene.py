"""CPU check of the plain part of csrc/track_scene.hpp (the front end of the entries that take cameras and a track CSR): the host compiler
alone builds tests/cpp/track_scene_test.cpp against the header, which is part of the check.  The program covers the lane classes at their
boundaries, the launch order, the estimated-only launch order of the outlier rule with each class empty in turn, and every refusal of the
track-array checks under each size rule and both settings of the track_ptr[0] check."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_classes_launch_order_and_track_array_checks(tmp_path):
    exe = str(tmp_path / "track_scene_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "track_scene_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
