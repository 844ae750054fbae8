#!/usr/bin/env python3
"""Times the full bundle adjustment -- orientations, positions and points (include/gsfm_ba6.h) -- on the synthetic scenes of
tools/time_bundle_adjustment.py (synth.make_tracks at the sizes of 1DSfM scenes).  Per size: wall ms of one solve (HUBER 10, from the
generator's scene perturbed by 0.05 on centres and points and 0.005 rad on the orientations), its LM and PCG iterations and stalled steps,
the same figures of the fixed-orientation solver (gsfm_ba_solve) from the same start -- free orientations worsen the conditioning of the
reduced system: PCG iterations per LM step, side by side -- and the mean device microseconds of the kernels of one linearisation and one
Schur product (gsfm_ba6_time_kernels) with a byte model against an HBM rate of 8 TB/s:
  point pass      100 B per observation (Jp, Jr 96, camera index 4) + 212 B per track (offsets, slot, S, the 3 x 3 inverse as a pair 144, z out) + 48 B per camera (q, gathered)
  camera pass     100 B per used observation (Jp, Jr 96, track index 4) + 24 B per track (z, gathered) + 248 B per camera
  lin, points     132 B per observation (camera index 4, pixel 16, Jp, Jr out 96, r~ out 16) + 116 B per track + 280 B per camera (record 256, position 24)
  lin, cameras    212 B per used observation (index 4, Jp, Jr in 96, r~ in 16, Jp, Jr out 96) + 224 B per camera
  cost            20 B per observation + 52 B per track + 152 B per camera
  preconditioner  100 B per used observation + 48 B per track (G_t, gathered) + 392 B per camera
  quadratic form  100 B per observation + 36 B per track + 48 B per camera (delta, gathered)
  camera records  304 B per camera
--focal: the same scene, start and run with free focal lengths as well (include/gsfm_ba7.h; the start's focal lengths are the generator's
times 1 + N(0, 0.01^2)): the solve's figures and gsfm_ba7_time_kernels under "focal_length", and per kernel the ratio to gsfm_ba6's time.
Its observations carry Jf too, 16 B more wherever Jp, Jr are read or written: the product passes predict 116 / 100 of the bytes above
(112 / 96 of the Jacobian stream).
Writes profiles/full_bundle_adjustment_times.json.
usage: tools/time_full_bundle_adjustment.py [--sizes 500x100k,5000x1M] [--reps 10] [--focal] [--out profiles/full_bundle_adjustment_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from globalsfmpy_amd import loss_functions as LF, synth  # noqa: E402
from globalsfmpy_amd.solver import BundleProblem, FocalBundleProblem, FullBundleProblem  # noqa: E402
from time_bundle_adjustment import HBM_BYTES_PER_US, parse  # noqa: E402
from time_triangulation import LENGTHS, WEIGHTS  # noqa: E402


def byte_model(N, T, O, U):
    return {"point_pass": 100 * O + 212 * T + 48 * N, "camera_pass": 100 * U + 24 * T + 248 * N, "lin_tracks": 132 * O + 116 * T + 280 * N,
            "lin_cameras": 212 * U + 224 * N, "cost": 20 * O + 52 * T + 152 * N, "preconditioner": 100 * U + 48 * T + 392 * N,
            "quadratic_form": 100 * O + 36 * T + 48 * N, "camera_records": 304 * N}


def byte_model_focal(N, T, O, U):
    """byte_model with Jf (16 B) beside every Jp, Jr, the focal coordinate's vectors (8 B per camera and vector, counted as 24: the node) and
    the 7 x 7 blocks"""
    m = byte_model(N, T, O, U)
    extra = {"point_pass": 16 * O + 24 * N, "camera_pass": 16 * U + 120 * N, "lin_tracks": 16 * O, "lin_cameras": 32 * U + 152 * N, "cost": 0,
             "preconditioner": 16 * U + 152 * N, "quadratic_form": 16 * O + 24 * N, "camera_records": 24 * N}
    return {k: m[k] + extra[k] for k in m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x100k,5000x1M")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--focal", action="store_true", help="also run and time the adjustment with free focal lengths (gsfm_ba7) on the same scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "full_bundle_adjustment_times.json"))
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        n_cams, n_tracks = parse(size)
        g = synth.make_tracks(n_cams, n_tracks, 31, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5, outlier_frac=0.02)
        N, T, O = n_cams, n_tracks, int(g["track_ptr"][-1])
        rng = np.random.default_rng(1)
        c0 = g["cam_pos"] + 0.05 * rng.standard_normal((N, 3))
        p0 = g["gt_points"] + 0.05 * rng.standard_normal((T, 3))
        w0 = g["rot_aa"] + 0.005 * rng.standard_normal((N, 3))
        t0 = time.perf_counter()
        P = FullBundleProblem(g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])
        P.set_loss(LF.HuberLoss(10.0))
        create_ms = 1e3 * (time.perf_counter() - t0)
        P.solve(w0, c0, p0, max_num_iterations=1)   # warm
        s = P.solve(w0, c0, p0)[3]
        us = P.time_kernels(w0, c0, p0, 1e4, a.reps)
        P.close()
        F = BundleProblem(w0, g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])   # the same start, its orientations held
        F.set_loss(LF.HuberLoss(10.0))
        F.solve(c0, p0, max_num_iterations=1)
        sf = F.solve(c0, p0)[2]
        F.close()
        model = byte_model(N, T, O, O)
        row = {"size": size, "n_cams": N, "n_tracks": T, "n_obs": O, "create_ms": create_ms, "solve_ms": s["t_total_ms"], "termination": s["termination_name"],
               "lm_iterations": s["num_iterations"], "pcg_iterations": s["num_cg_iterations"], "pcg_stalled_steps": s["num_pcg_stalled_steps"],
               "initial_cost": s["initial_cost"], "final_cost": s["final_cost"],
               "ms_per_pcg_iteration_wall": s["t_total_ms"] / max(1, s["num_cg_iterations"]),
               "pcg_iterations_per_lm_step": s["num_cg_iterations"] / max(1, s["num_iterations"]),
               "fixed_orientation": {"solve_ms": sf["t_total_ms"], "termination": sf["termination_name"], "lm_iterations": sf["num_iterations"],
                                     "pcg_iterations": sf["num_cg_iterations"], "pcg_stalled_steps": sf["num_pcg_stalled_steps"],
                                     "final_cost": sf["final_cost"], "pcg_iterations_per_lm_step": sf["num_cg_iterations"] / max(1, sf["num_iterations"]),
                                     "ms_per_pcg_iteration_wall": sf["t_total_ms"] / max(1, sf["num_cg_iterations"])},
               "kernels": {k: {"us": float(v), "model_bytes": model[k], "floor_us_at_8TBps": model[k] / HBM_BYTES_PER_US,
                               "fraction_of_8TBps": model[k] / HBM_BYTES_PER_US / v if v > 0 else None} for k, v in us.items()}}
        if a.focal:
            f0 = g["intrinsics"][:, 0] * (1 + 0.01 * rng.standard_normal(N))
            Q = FocalBundleProblem(g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])
            Q.set_loss(LF.HuberLoss(10.0))
            Q.solve(w0, c0, f0, p0, max_num_iterations=1)   # warm
            sq = Q.solve(w0, c0, f0, p0)[4]
            uq = Q.time_kernels(w0, c0, f0, p0, 1e4, a.reps)
            Q.close()
            mq = byte_model_focal(N, T, O, O)
            row["focal_length"] = {"solve_ms": sq["t_total_ms"], "termination": sq["termination_name"], "lm_iterations": sq["num_iterations"],
                                   "pcg_iterations": sq["num_cg_iterations"], "pcg_stalled_steps": sq["num_pcg_stalled_steps"],
                                   "initial_cost": sq["initial_cost"], "final_cost": sq["final_cost"],
                                   "pcg_iterations_per_lm_step": sq["num_cg_iterations"] / max(1, sq["num_iterations"]),
                                   "ms_per_pcg_iteration_wall": sq["t_total_ms"] / max(1, sq["num_cg_iterations"]),
                                   "kernels": {k: {"us": float(v), "ratio_to_ba6": float(v) / us[k] if us[k] > 0 else None, "model_bytes": mq[k],
                                                   "model_ratio_to_ba6": mq[k] / model[k], "fraction_of_8TBps": mq[k] / HBM_BYTES_PER_US / v if v > 0 else None}
                                               for k, v in uq.items()}}
            for k in us:
                print("%-16s ba6 %10.1f us   ba7 %10.1f us   ratio %.3f (bytes predict %.3f)" % (k, us[k], uq[k], uq[k] / us[k], mq[k] / model[k]), flush=True)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
