#!/usr/bin/env python3
"""Times position estimation with point-to-camera constraints (include/gsfm_posp.h) on synthetic scenes of synth.make_position_scene.
Per size: wall ms of problem creation and of one solve (HUBER 0.1, the reference's start: cameras at 0, points at (1, 1, 1)), its LM and PCG
iterations, and the mean device microseconds of the kernels of one linearisation and one product with the reduced camera operator
(gsfm_posp_time_kernels) with a byte model against an HBM rate of 8 TB/s (E edges, O observations, U used ones, T tracks, N cameras):
  rays            52 B per observation (camera index 4, pixel 16, flag 1 + padding, ray out 24) + 48 B per camera (angle-axis, intrinsics; gathered)
  lin, tracks     100 B per observation (camera index 4, ray 24, block out 48, a out 24) + 116 B per track + 25 B per camera (position, flag; gathered)
  lin, cameras    2 E x 76 B (neighbour 4, direction 24, block out 48) + 124 B per used observation (index 4, block in 48, a in 24, block out 48) + 104 B per camera
  cost, tracks    28 B per observation + 52 B per track + 25 B per camera
  point pass      52 B per observation (block 48, camera index 4) + 140 B per track + 24 B per camera (q, gathered)       (ba_kernels.hpp's kernel)
  camera pass     2 E x 52 B (block 48, neighbour 4) + 52 B per used observation + 24 B per track (z, gathered) + 128 B per camera
  preconditioner  2 E x 48 B + 100 B per used observation (block 48, track index 4, G_t 48) + 136 B per camera
Writes profiles/position_points_times.json.
usage: tools/time_position_points.py [--sizes 500x5000x20k,5000x50000x200k] [--reps 10] [--out profiles/position_points_times.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from globalsfmpy_amd import loss_functions as LF, synth  # noqa: E402
from globalsfmpy_amd.solver import PointPositionProblem  # noqa: E402

HBM_BYTES_PER_US = 8e6   # 8 TB/s


def byte_model(N, E, T, O, U):
    return {"rays": 52 * O + 48 * N, "lin_tracks": 100 * O + 116 * T + 25 * N, "lin_cameras": 152 * E + 124 * U + 104 * N,
            "cost_tracks": 28 * O + 52 * T + 25 * N, "point_pass": 52 * O + 140 * T + 24 * N, "camera_pass": 104 * E + 52 * U + 24 * T + 128 * N,
            "preconditioner": 96 * E + 100 * U + 136 * N}


def number(text):
    mult = {"k": 1000, "m": 1000000}
    text = text.lower()
    return int(float(text[:-1]) * mult[text[-1]]) if text[-1] in mult else int(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x5000x20k,5000x50000x200k", help="cameras x edges x tracks, comma separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_points_times.json"))
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        n_cams, n_edges, n_tracks = (number(v) for v in size.split("x"))
        g = synth.make_position_scene(n_cams, n_edges, n_tracks, 31, lengths=(2, 3, 4, 5, 8, 13), noise=0.005, outlier_frac=0.1)
        N, E, T, O = n_cams, len(g["edge_i"]), n_tracks, int(g["track_ptr"][-1])
        t0 = time.perf_counter()
        P = PointPositionProblem(N, g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], g["rot_aa"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"],
                                 a.weight * E / O)
        P.set_loss(LF.HuberLoss(0.1))
        create_ms = 1e3 * (time.perf_counter() - t0)
        P.solve(max_num_iterations=1)   # warm
        _, _, s = P.solve()
        us = P.time_kernels(g["gt_pos"], g["gt_points"], 1e4, a.reps)
        model = byte_model(N, E, T, O, s["num_observations_used"])
        row = {"size": size, "n_cams": N, "n_edges": E, "n_tracks": T, "n_obs": O, "n_obs_used": s["num_observations_used"], "active_points": s["num_active_points"],
               "create_ms": create_ms, "solve_ms": s["t_total_ms"], "termination": s["termination_name"], "lm_iterations": s["num_iterations"],
               "pcg_iterations": s["num_cg_iterations"], "pcg_stalled_steps": s["num_pcg_stalled_steps"], "initial_cost": s["initial_cost"], "final_cost": s["final_cost"],
               "ms_per_pcg_iteration_wall": s["t_total_ms"] / max(1, s["num_cg_iterations"]),
               "kernels": {k: {"us": float(v), "model_bytes": model[k], "floor_us_at_8TBps": model[k] / HBM_BYTES_PER_US,
                               "fraction_of_8TBps": model[k] / HBM_BYTES_PER_US / v if v > 0 else None} for k, v in us.items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
        P.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
