"""The maximum-spanning-tree initialisation on the C5 graph (100k cameras, 10M edges, 30 % outliers): the device entry point
(gsfm_rot_init_spanning_tree) against the scipy construction of synth.spanning_tree_init, then a solve from the device's start.
Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from globalsfmpy_amd import _abi, synth  # noqa: E402
from globalsfmpy_amd import loss_functions as LF  # noqa: E402
from globalsfmpy_amd.solver import RotationProblem, edge_sq_norms, orientations_from_maximum_spanning_tree  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    g = synth.make_graph(a.cams, a.edges, seed=a.seed, outlier_frac=0.3)
    t0 = time.perf_counter()
    init_ref, matches = synth.spanning_tree_init(g, a.seed)      # scipy tree + host composition, as bench.py times it
    t_scipy = time.perf_counter() - t0
    n, ei, ej, rel = g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"]
    w = matches.astype(np.int32)
    t0 = time.perf_counter()
    cold = orientations_from_maximum_spanning_tree(n, ei, ej, rel, w)
    cold_ms = 1e3 * (time.perf_counter() - t0)
    wall, kern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = orientations_from_maximum_spanning_tree(n, ei, ej, rel, w)
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(out["kernel_ms"])
    e = out["parent_edge"][out["parent_edge"] >= 0]
    t = minimum_spanning_tree(sp.coo_matrix((-matches.astype(np.float64), (ei.astype(np.int64), ej.astype(np.int64))), shape=(n, n)).tocsr())
    loop = np.sqrt(edge_sq_norms(n, ei[e], ej[e], rel[e], out["rot_aa"])["s"].max())
    err_dev = synth.angular_distance(synth.align_rotations(out["rot_aa"], g["gt_aa"]), g["gt_aa"])
    err_ref = synth.angular_distance(synth.align_rotations(init_ref, g["gt_aa"]), g["gt_aa"])
    # end to end from host arrays: init + problem creation + one solve from that start
    t0 = time.perf_counter()
    o2 = orientations_from_maximum_spanning_tree(n, ei, ej, rel, w)
    t_init = time.perf_counter()
    prob = RotationProblem(n, ei, ej, rel, _abi.ANGLE_AXIS_COVARIANCE, cov6=g["cov6"])
    prob.set_loss(LF.MAGSACWeightBasedLoss(0.02))
    t_create = time.perf_counter()
    rot, st = prob.solve(o2["rot_aa"])
    t_end = time.perf_counter()
    t1 = time.perf_counter()
    _, st_warm = prob.solve(o2["rot_aa"])
    solve_warm_ms = 1e3 * (time.perf_counter() - t1)
    _, st_ref = prob.solve(init_ref)
    err_sol = synth.angular_distance(synth.align_rotations(rot, g["gt_aa"]), g["gt_aa"])
    res = {
        "graph": "synth.make_graph(%d, %d, seed=%d, outlier_frac=0.3); weights = synth.spanning_tree_init's match counts" % (a.cams, a.edges, a.seed),
        "device_cold_wall_ms": cold_ms, "device_cold_kernel_ms": cold["kernel_ms"],
        "device_warm_wall_ms_median": float(np.median(wall)), "device_warm_kernel_ms_median": float(np.median(kern)), "reps": a.reps,
        "scipy_spanning_tree_init_s": t_scipy,
        "tree_weight": int(w[e].sum()), "scipy_mst_weight": int(round(-t.sum())),
        "n_tree_cams": out["n_tree_cams"], "root": out["root"], "depth": out["depth"],
        "max_tree_edge_loop_angle_rad": float(loop),
        "init_mean_error_vs_ground_truth_deg": float(np.rad2deg(err_dev.mean())),
        "scipy_init_mean_error_vs_ground_truth_deg": float(np.rad2deg(err_ref.mean())),
        "end_to_end_ms": 1e3 * (t_end - t0),
        "end_to_end_phases_ms": {"init": 1e3 * (t_init - t0), "problem_create": 1e3 * (t_create - t_init), "solve": 1e3 * (t_end - t_create)},
        "solve_warm_ms": solve_warm_ms,
        "solve_from_device_tree": {"lm_iterations": st["num_iterations"], "termination": st["termination_name"], "final_cost": st["final_cost"],
                                   "mean_error_vs_ground_truth_deg": float(np.rad2deg(err_sol.mean()))},
        "solve_from_scipy_tree": {"lm_iterations": st_ref["num_iterations"], "termination": st_ref["termination_name"], "final_cost": st_ref["final_cost"]},
        "solve_warm_termination": st_warm["termination_name"],
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
