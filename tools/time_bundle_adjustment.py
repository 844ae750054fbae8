#!/usr/bin/env python3
"""Times the bundle adjustment of camera positions and points (include/gsfm_ba.h) on synthetic scenes of synth.make_tracks at the sizes of
1DSfM scenes.  Per size: wall ms of one solve (HUBER 10, from the generator's scene perturbed by 0.05), its LM and PCG iterations, and the
mean device microseconds of the kernels of one linearisation and one Schur product (gsfm_ba_time_kernels) with a byte model against an
HBM rate of 8 TB/s:
  point pass      52 B per observation (block 48, camera index 4) + 140 B per track (offsets, slot, S, the 3 x 3 inverse, z out) + 24 B per camera (q, gathered)
  camera pass     52 B per used observation (block 48, track index 4) + 24 B per track (z, gathered) + 128 B per camera
  lin, points     92 B per observation (camera index 4, pixel 16, block out 48, a out 24) + 116 B per track + 152 B per camera (record, position)
  lin, cameras    124 B per used observation (index 4, block in 48, a in 24, block out 48) + 80 B per camera
  cost            20 B per observation + 52 B per track + 152 B per camera
The reference tier's (tests/ba_reference.py, numpy fp64) solve of the 70-camera test scene is timed beside it as context.
Writes profiles/bundle_adjustment_times.json.
usage: tools/time_bundle_adjustment.py [--sizes 500x100k,5000x1M] [--reps 10] [--out profiles/bundle_adjustment_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from globalsfmpy_amd import loss_functions as LF, synth  # noqa: E402
from globalsfmpy_amd.solver import BundleProblem  # noqa: E402
from time_triangulation import LENGTHS, WEIGHTS  # noqa: E402

HBM_BYTES_PER_US = 8e6   # 8 TB/s


def byte_model(N, T, O, U):
    return {"point_pass": 52 * O + 140 * T + 24 * N, "camera_pass": 52 * U + 24 * T + 128 * N, "lin_tracks": 92 * O + 116 * T + 152 * N,
            "lin_cameras": 124 * U + 80 * N, "cost": 20 * O + 52 * T + 152 * N}


def parse(size):
    cams, tracks = size.lower().split("x")
    mult = {"k": 1000, "m": 1000000}
    return int(cams), int(float(tracks[:-1]) * mult[tracks[-1]]) if tracks[-1] in mult else int(tracks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x100k,5000x1M")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_adjustment_times.json"))
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        n_cams, n_tracks = parse(size)
        g = synth.make_tracks(n_cams, n_tracks, 31, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5, outlier_frac=0.02)
        N, T, O = n_cams, n_tracks, int(g["track_ptr"][-1])
        rng = np.random.default_rng(1)
        c0 = g["cam_pos"] + 0.05 * rng.standard_normal((N, 3))
        p0 = g["gt_points"] + 0.05 * rng.standard_normal((T, 3))
        t0 = time.perf_counter()
        P = BundleProblem(g["rot_aa"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])
        P.set_loss(LF.HuberLoss(10.0))
        create_ms = 1e3 * (time.perf_counter() - t0)
        P.solve(c0, p0, max_num_iterations=1)   # warm
        _, _, s = P.solve(c0, p0)
        us = P.time_kernels(c0, p0, 1e4, a.reps)
        model = byte_model(N, T, O, O)
        row = {"size": size, "n_cams": N, "n_tracks": T, "n_obs": O, "create_ms": create_ms, "solve_ms": s["t_total_ms"], "termination": s["termination_name"],
               "lm_iterations": s["num_iterations"], "pcg_iterations": s["num_cg_iterations"], "initial_cost": s["initial_cost"], "final_cost": s["final_cost"],
               "ms_per_pcg_iteration_wall": s["t_total_ms"] / max(1, s["num_cg_iterations"]),
               "kernels": {k: {"us": float(v), "model_bytes": model.get(k), "floor_us_at_8TBps": model[k] / HBM_BYTES_PER_US if k in model else None,
                               "fraction_of_8TBps": model[k] / HBM_BYTES_PER_US / v if k in model and v > 0 else None} for k, v in us.items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
        P.close()
    if not a.no_reference:
        import ba_reference as R
        sc = R.scene("b")
        c0, p0 = R.case_start("b_near")
        t0 = time.perf_counter()
        o = R.lm_solve(sc, c0, p0, "huber", 10.0)
        ref_ms = 1e3 * (time.perf_counter() - t0)
        P = BundleProblem(sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"])
        P.set_loss(LF.HuberLoss(10.0))
        P.solve(c0, p0)
        _, _, s = P.solve(c0, p0)
        row = {"size": "test scene b (70 cameras, %d tracks, %d observations)" % (len(sc["pt_est"]), len(sc["obs_cam"])), "reference_numpy_solve_ms": ref_ms,
               "reference_lm_iterations": o["iterations"], "solve_ms": s["t_total_ms"], "lm_iterations": s["num_iterations"], "pcg_iterations": s["num_cg_iterations"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
