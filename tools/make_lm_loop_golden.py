#!/usr/bin/env python3
"""Records the bytes that gsfm_ba6_solve and gsfm_pos_solve return, for the parent-bytes tests of tests/test_gpu_ba6.py and
tests/test_gpu_positions.py.  Run on the GPU with GSFM_ROT_LIB pointing at a library built from the commit whose bytes are to be kept (the
one before the solvers' host loops moved to csrc/lm_loop.hpp):

    GSFM_ROT_LIB=/path/to/parent/libgsfm_rot.so python tools/make_lm_loop_golden.py [--out-dir tests/golden]

Writes ba6_solve_parent_bytes.npz (scene b from case_start("b_near") and scene a from case_start("a_far") of tests/ba6_reference.py, Huber 10:
<case>_rot, _cam, _points, _final_cost, _counts) and pos_solve_parent_bytes.npz (synth.make_position_graph(60, 500, seed=11,
outlier_frac=0.3, noise=0.01), Huber 0.1, fixed_cam=0, from the start array `start` of the file; dense_*: Cholesky steps, pcg_*:
dense_max_cams=0).  counts: termination, iterations, successful and unsuccessful steps, PCG iterations (positions: and dense solves)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import _abi, loss_functions as LF, synth  # noqa: E402
from globalsfmpy_amd.solver import FullBundleProblem, PositionProblem  # noqa: E402
import ba6_reference as R  # noqa: E402

COUNTS = ["termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_cg_iterations"]


def position_start(g):
    return g["gt_pos"] + np.random.default_rng(5).normal(0.0, 1.0, g["gt_pos"].shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    print("library: %s" % _abi.LIB_PATH)
    ba6 = {}
    for name in ("b_near", "a_far"):
        sc = R.scene(R.CASES[name][0])
        w0, c0, p0 = R.split(sc, R.case_start(name))
        P = FullBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"])
        P.set_loss(LF.HuberLoss(10.0))
        w1, c1, p1, s = P.solve(w0, c0, p0)
        ba6.update({name + "_rot": w1, name + "_cam": c1, name + "_points": p1, name + "_final_cost": np.array([s["final_cost"]]),
                    name + "_counts": np.array([s[k] for k in COUNTS], dtype=np.int64)})
        print(name, s["termination_name"], [s[k] for k in COUNTS], "final cost %.17g" % s["final_cost"])
    assert ba6["a_far_counts"][3] > 0, "the far start takes no rejected step: record another far case"
    np.savez(os.path.join(a.out_dir, "ba6_solve_parent_bytes.npz"), **ba6)

    g = synth.make_position_graph(60, 500, seed=11, outlier_frac=0.3, noise=0.01)
    pos = {"start": position_start(g)}
    for tag, options in (("dense", {}), ("pcg", {"dense_max_cams": 0})):
        P = PositionProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"])
        P.set_loss(LF.HuberLoss(0.1))
        x, s = P.solve(pos["start"], fixed_cam=0, **options)
        counts = [s[k] for k in COUNTS + ["num_dense_solves"]]
        assert (s["num_dense_solves"] > 0) == (tag == "dense") and (s["num_cg_iterations"] > 0) == (tag == "pcg"), s
        pos.update({tag + "_pos": x, tag + "_final_cost": np.array([s["final_cost"]]), tag + "_counts": np.array(counts, dtype=np.int64)})
        print("positions", tag, s["termination_name"], counts, "final cost %.17g" % s["final_cost"])
    np.savez(os.path.join(a.out_dir, "pos_solve_parent_bytes.npz"), **pos)


if __name__ == "__main__":
    main()
