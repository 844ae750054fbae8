#!/usr/bin/env python3
"""Records the bytes that gsfm_ba7_solve and the step checks of both full bundle adjustments return, for the parent-bytes tests of
tests/test_gpu_ba7.py and tests/test_gpu_full_ba_step_bytes.py.  Run on the GPU with GSFM_ROT_LIB pointing at a library built from the commit
whose bytes are to be kept (the one before the 6- and 7-coordinate solvers became one kernel family and one host template):

    GSFM_ROT_LIB=/path/to/parent/libgsfm_rot.so python tools/make_full_ba_parent_golden.py [--out-dir tests/golden]

Writes ba7_solve_parent_bytes.npz (tests/ba7_reference.py under Huber 10: a_near, a far case that takes a rejected step, and a_near with the
MIXED focal mask of tests/test_gpu_ba7.py as a_near_mixed: <case>_rot, _cam, _focal, _points, _final_cost, _counts; far_case names the far
case) and full_ba_step_parent_bytes.npz (every output of step_check at the default options for STEP_CASES from the near starts of the step
tests, ba6_<case>_* from FullBundleProblem and ba7_<case>_* from FocalBundleProblem: the arrays of STEP_ARRAYS, _scal = model cost change,
delta.g, |J delta|^2, the PCG's relative residual, _info = PCG iterations, stalled).  counts: termination, iterations, successful and
unsuccessful steps, PCG iterations."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import _abi, loss_functions as LF  # noqa: E402
from globalsfmpy_amd.solver import FocalBundleProblem, FullBundleProblem  # noqa: E402
import ba6_reference as R6  # noqa: E402
import ba7_reference as R7  # noqa: E402

COUNTS = ["termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_cg_iterations"]
MIXED = np.arange(12) % 3 != 1   # tests/test_gpu_ba7.py
STEP_CASES = {"t_tukey_1e10": ("t", "tukey", 1e10), "t_tukey_1e4": ("t", "tukey", 1e4), "a_huber_1e4": ("a", "huber", 1e4)}
STEP_ARRAYS = {"ba6": ["rhs", "y_cam", "y_point", "delta_rot", "delta_pos", "delta_point", "j_delta"],
               "ba7": ["rhs", "y_cam", "y_point", "delta_rot", "delta_pos", "delta_focal", "delta_point", "j_delta"]}


def step_loss(lname):
    return {"tukey": LF.TukeyLoss(10.0), "huber": LF.HuberLoss(10.0)}[lname]


def focal_problem(sc, loss):
    P = FocalBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"], sc["focal_free"])
    P.set_loss(loss)
    return P


def focal_start(sc, x):
    w, c, p = R7.split(sc, x)
    return np.array(w), np.array(c), np.array(R7.focal_of(sc, x)), np.array(p)


def solve_case(name, focal_free=None):
    sc = R7.scene(R7.CASES[name][0], focal_free)
    w, c, f, p, s = focal_problem(sc, LF.HuberLoss(10.0)).solve(*focal_start(sc, R7.case_start(name)))
    print(name, "mixed" if focal_free is not None else "", s["termination_name"], [s[k] for k in COUNTS], "final cost %.17g" % s["final_cost"])
    return {"rot": w, "cam": c, "focal": f, "points": p, "final_cost": np.array([s["final_cost"]]), "counts": np.array([s[k] for k in COUNTS], dtype=np.int64)}


def step_case(solver, sname, lname, radius):
    """step_check's outputs from the near start of tests/test_gpu_ba6.py's and tests/test_gpu_ba7.py's step tests"""
    if solver == "ba6":
        sc = R6.scene(sname)
        P = FullBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"])
        P.set_loss(step_loss(lname))
        st = P.step_check(*R6.split(sc, R6.near_start(sname)), radius)
    else:
        sc = R7.scene(sname)
        st = focal_problem(sc, step_loss(lname)).step_check(*focal_start(sc, R7.near_start(sname)), radius)
    out = {k: st[k] for k in STEP_ARRAYS[solver]}
    out["scal"] = np.array([st["model_cost_change"], st["dg"], st["jd2"], st["cg_rel"]])
    out["info"] = np.array([st["cg_iterations"], int(st["stalled"])], dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    print("library: %s" % _abi.LIB_PATH)
    ba7 = {}
    for key, got in (("a_near", solve_case("a_near")), ("a_near_mixed", solve_case("a_near", MIXED))):
        ba7.update({key + "_" + k: v for k, v in got.items()})
    for far in ("a_far", "b_far", "c_far", "t_far"):
        got = solve_case(far)
        if got["counts"][3] > 0:
            break
    assert got["counts"][3] > 0, "no far start takes a rejected step"
    ba7.update({far + "_" + k: v for k, v in got.items()})
    ba7["far_case"] = np.array(far)
    np.savez(os.path.join(a.out_dir, "ba7_solve_parent_bytes.npz"), **ba7)

    steps = {}
    for solver in ("ba6", "ba7"):
        for case, (sname, lname, radius) in STEP_CASES.items():
            got = step_case(solver, sname, lname, radius)
            print(solver, case, "PCG", list(got["info"]), "scalars", ["%.17g" % v for v in got["scal"]])
            steps.update({"%s_%s_%s" % (solver, case, k): v for k, v in got.items()})
    np.savez(os.path.join(a.out_dir, "full_ba_step_parent_bytes.npz"), **steps)


if __name__ == "__main__":
    main()
