#!/usr/bin/env python3
"""The robust L1 + IRLS rotation estimator (include/gsfm_rot_l1l2.h) at benchmark scale: synth.make_graph at 10 000 cameras / 200 000
edges and at 100 000 / 10 000 000 (seed 2023: the rotation and position benchmarks' edge set), 20 % outliers, started at the graph's
init_aa, camera 0 fixed.  Prints one JSON line per size:
  call time and kernel_ms (median and range over --steps calls), stage counts, time per ADMM iteration and per PCG iteration,
  the Laplacian product alone (the aid's own timer: 20 launches back to back), its bytes from the shapes and the fraction of 8 TB/s,
  its time per directed entry beside that of a PCG iteration of the position solver on the same graph (whose mat-vec k_pos_matvec
  is 92 % of it: DESIGN.md, section 11),
  the mean angular error to the ground truth (after alignment) beside that of gsfm_rot_solve with MAGSACWeightBasedLoss(0.02) from the
  same start, and, for the smaller size, the wall time of the scipy restatement (tests/robust_rotation_reference.py, sparse LU).
  python tools/time_robust_rotations.py [--sizes small large] [--steps K] [--no-position] [--no-scipy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12
SIZES = {"small": (10000, 200000), "large": (100000, 10000000)}


def spread(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def mean_error_deg(synth, rot, gt):
    return float(np.degrees(np.mean(synth.angular_distance(synth.align_rotations(rot, gt), gt))))


def run(name, args):
    from globalsfmpy_amd import _abi, solver, synth
    from globalsfmpy_amd import loss_functions as lf
    n, e = SIZES[name]
    g = synth.make_graph(n_cams=n, n_edges=e, seed=2023, outlier_frac=0.2)
    ei, ej, rel, init, gt = g["edge_i"], g["edge_j"], g["rel_aa"], g["init_aa"], g["gt_aa"]
    out = {"metric": "robust_l1l2_rotations", "n_cams": n, "n_edges": int(ei.shape[0]), "outliers": 0.2}
    call_ms, kernel_ms, s, rot = [], [], None, None
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        rot, s = solver.estimate_rotations_robust_l1l2(n, ei, ej, rel, init, 0)
        if k >= args.warmup:
            call_ms.append((time.perf_counter() - t0) * 1e3); kernel_ms.append(s["kernel_ms"])
    admm = sum(s["num_admm_iterations"])
    out.update({"call_ms": spread(call_ms), "kernel_ms": spread(kernel_ms), "admm_iterations": s["num_admm_iterations"],
                "l1_step": [round(v, 6) for v in s["l1_step"]], "irls_iterations": s["num_irls_iterations"], "cg_iterations": s["num_cg_iterations"],
                "linear_solves": s["num_linear_solves"], "stalled_solves": s["num_pcg_stalled_solves"],
                "worst_cg_residual": s["worst_accepted_cg_residual"],
                # an ADMM iteration is its solve and its two sweeps; the whole call over the iterations of both stages bounds it from above
                "ms_per_admm_iteration_incl_solve": round(spread(kernel_ms)["median"] / max(1, admm + s["num_irls_iterations"]), 4),
                "ms_per_cg_iteration_whole_call": round(spread(kernel_ms)["median"] / max(1, s["num_cg_iterations"]), 5),
                "mean_error_deg": round(mean_error_deg(synth, rot, gt), 4)})
    # the PCG and the product alone, both forms, on a random right-hand side
    rng = np.random.default_rng(1)
    rhs = rng.standard_normal((n, 3))
    w = np.exp(rng.uniform(np.log(1e-3), np.log(1.5e3), ei.shape[0]))
    for form, weights in (("unit", None), ("weighted", w)):
        prod, per_it = [], []
        for _ in range(args.steps):
            _, info = solver.robust_l1l2_laplacian_solve(n, ei, ej, rhs, weights, 0)
            prod.append(info["product_ms"] * 1e3); per_it.append(info["kernel_ms"] / max(1, info["cg_iterations"]) * 1e3)
        us = spread(prod)["median"]
        out["product_" + form] = {"us": spread(prod), "bytes": info["product_bytes"], "of_8TBps": round(info["product_bytes"] / (us * 1e-6) / HBM, 4),
                                  "ps_per_directed_entry": round(us * 1e6 / (2 * ei.shape[0]), 3), "us_per_cg_iteration": spread(per_it),
                                  "cg_iterations": info["cg_iterations"]}
    # the nonlinear solver with the MAGSAC loss from the same start
    from globalsfmpy_amd.solver import RotationProblem
    p = RotationProblem(n, ei, ej, rel, _abi.ANGLE_AXIS_COVARIANCE, cov6=g["cov6"])
    p.set_loss(lf.MAGSACWeightBasedLoss(0.02))
    t0 = time.perf_counter()
    rot_m, sm = p.solve(init)
    out["magsac_nonlinear"] = {"mean_error_deg": round(mean_error_deg(synth, rot_m, gt), 4), "call_ms": round((time.perf_counter() - t0) * 1e3, 2),
                               "lm_iterations": sm["num_iterations"]}
    p.close()
    if not args.no_position:   # the position solver's PCG on the same edges: its iteration is k_pos_matvec plus six small kernels
        from globalsfmpy_amd.solver import PositionProblem
        pg = synth.make_position_graph(n, e, 2023, outlier_frac=0.2, noise=0.01)
        pp = PositionProblem(pg["n_cams"], pg["edge_i"], pg["edge_j"], pg["rel_t"], pg["rot_aa"])
        pp.set_loss(lf.HuberLoss(0.1))
        _, ps = pp.solve(None, fixed_cam=0, dense_max_cams=0, max_num_iterations=2)
        if ps["num_cg_iterations"] > 0:
            us = ps["t_total_ms"] / ps["num_cg_iterations"] * 1e3
            out["position_pcg"] = {"us_per_cg_iteration_whole_call": round(us, 2), "cg_iterations": ps["num_cg_iterations"],
                                   "ps_per_directed_entry": round(us * 1e6 / (2 * pg["edge_i"].shape[0]), 3)}
        pp.close()
    if name == "small" and not args.no_scipy:
        import robust_rotation_reference as ref
        t0 = time.perf_counter()
        rot_r, log = ref.solve(n, ei, ej, rel, init, 0, linear="direct")
        out["scipy_restatement"] = {"wall_s": round(time.perf_counter() - t0, 2), "admm_iterations": log["admm_iterations"], "irls_iterations": log["irls_iterations"],
                                    "max_abs_difference_rad": float(np.abs(rot_r - rot).max()), "margin": log["margin"]}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["small", "large"], choices=sorted(SIZES))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-position", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    for name in args.sizes:
        run(name, args)


if __name__ == "__main__":
    main()
