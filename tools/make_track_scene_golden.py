#!/usr/bin/env python3
"""Records the bytes that gsfm_tracks_outlier_tracks returns, for the parent-bytes test of tests/test_gpu_outlier_tracks.py.  Run on the GPU
with GSFM_ROT_LIB pointing at a library built from the commit whose bytes are to be kept (the one before the track front ends moved to
csrc/track_scene.hpp):

    GSFM_ROT_LIB=/path/to/parent/libgsfm_rot.so python tools/make_track_scene_golden.py [--out-dir tests/golden]

Writes outlier_parent_bytes.npz: <case>_status, _n_views, _mean_sq_err, _counts for the cases of test_gpu_outlier_tracks.parent_bytes_cases --
outlier_reference.make_batch() with every track estimated as the batch has it, with the half-flagged mask of
test_another_track_s_flag_changes_nothing, and its tracks of one lane class alone (4, 16, 64 lanes: the other two classes are empty).
Also checks that the library returns the bytes of tests/golden/ba_fixed_orientation_scene_b.npz (gsfm_ba_solve on scene b of
tests/ba_reference.py, Huber 10, the b_near start), so that test_gpu_ba6.py's test of that file is a parent-bytes test of this commit too."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import _abi, loss_functions as LF  # noqa: E402
from globalsfmpy_amd.solver import BundleProblem  # noqa: E402
import ba_reference as B  # noqa: E402
import outlier_reference as out  # noqa: E402
import test_gpu_outlier_tracks as T  # noqa: E402

COUNTS = ["termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_cg_iterations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    print("library: %s" % _abi.LIB_PATH)
    doc = {}
    for name, scene in T.parent_bytes_cases(out.make_batch()):
        r = T.run(scene)
        doc.update({name + "_" + k: r[k] for k in T.OUTPUTS + ("counts",)})
        print("%-12s %5d tracks, counts %s, %.3f ms" % (name, len(r["status"]), list(r["counts"]), r["kernel_ms"]))
    np.savez(os.path.join(a.out_dir, "outlier_parent_bytes.npz"), **doc)

    gold = np.load(os.path.join(ROOT, "tests", "golden", "ba_fixed_orientation_scene_b.npz"))
    sc = B.scene("b")
    c0, p0 = B.case_start("b_near")
    P = BundleProblem(sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"])
    P.set_loss(LF.HuberLoss(10.0))
    c1, p1, s = P.solve(c0, p0)
    same = (c1.tobytes() == gold["cam_pos"].tobytes() and p1.tobytes() == gold["points"].tobytes() and s["final_cost"] == gold["final_cost"][0] and
            [s[k] for k in COUNTS] == list(gold["counts"]))
    print("gsfm_ba_solve, scene b: %s, final cost %.17g: %s ba_fixed_orientation_scene_b.npz" % ([s[k] for k in COUNTS], s["final_cost"],
                                                                                             "the bytes of" if same else "NOT the bytes of"))
    assert same


if __name__ == "__main__":
    main()
