#!/usr/bin/env python3
"""Times the track selection for bundle adjustment (gsfm_tracks_select_good, include/gsfm_tracks.h) on synthetic scenes of
tools/time_outlier_tracks.py's kind (synth.make_tracks; 0.5 px noise, 2 % gross outliers; the points are the generator's plus the
bundle-adjustment tools' 0.05 start offset): the 500-camera size of that tool and one of 1 000 cameras.  Per scene, warm medians of --reps
calls after one warm-up call:
  the device call      wall time from host arrays, HIP-event kernel time, the number of items downloaded for the top-up and the host's replay;
  a deficient setting  the same call with 1 000 tracks per view, under which cameras need the top-up (with 100 none does on these scenes);
  the host baseline    gsfm_tracks_select_good_from_statistics fed with the device's statistics (it does not compute them), and whether its
                       bytes equal the device's;
  the adjustment       one gsfm_ba6_solve (HUBER 10) over all tracks and one over the selected tracks only, wall time and iterations.
The parameters are the reference's flag files': threshold 10, cells of 100 pixels, 100 tracks per view.  Writes profiles/track_selection.json.
usage: tools/time_track_selection.py [--reps 7] [--sizes 500x100k,1000x200k] [--no-adjustment] [--out profiles/track_selection.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from globalsfmpy_amd import loss_functions as LF  # noqa: E402
from globalsfmpy_amd import synth  # noqa: E402
from globalsfmpy_amd.solver import FullBundleProblem, select_good_tracks, select_good_tracks_from_statistics  # noqa: E402
from time_bundle_adjustment import parse  # noqa: E402
from time_triangulation import LENGTHS, WEIGHTS  # noqa: E402

L, S, K = 10, 100, 100
K_DEFICIENT = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x100k,1000x200k")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-adjustment", action="store_true", help="skip the two bundle adjustments")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_selection.json"))
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
        args = (g["rot_aa"], g["cam_pos"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"], p0)
        kw = dict(long_track_length_threshold=L, image_grid_cell_size_pixels=S, min_num_optimized_tracks_per_view=K)
        r = select_good_tracks(*args, **kw)   # warm-up
        wall, kern, replay = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = select_good_tracks(*args, **kw)
            wall.append(1e3 * (time.perf_counter() - t0)); kern.append(r["kernel_ms"]); replay.append(r["replay_ms"])
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            h = select_good_tracks_from_statistics(N, g["track_ptr"], g["obs_cam"], g["obs_xy"], r["n_views"], r["mean_sq_err"], **kw)
            host.append(1e3 * (time.perf_counter() - t0))
        row = {"size": size, "n_cams": N, "n_tracks": T, "n_obs": O, "reps": a.reps, "parameters": {"long_track_length_threshold": L, "cell_size_pixels": S, "min_tracks_per_view": K},
               "device_wall_ms_median": float(np.median(wall)), "device_kernel_ms_median": float(np.median(kern)), "device_wall_ms": wall, "device_kernel_ms": kern,
               "deficient_items": r["deficient_items"], "deficient_list_bytes": 12 * r["deficient_items"], "host_replay_ms_median": float(np.median(replay)),
               "host_baseline_ms_median": float(np.median(host)), "host_baseline_ms": host,
               "host_baseline_equals_device": bool(np.array_equal(h["selected"], r["selected"]) and h["counts"] == r["counts"]),
               "counts": r["counts"], "share_of_tracks_selected": r["counts"]["selected"] / max(1, r["counts"]["tracks_with_items"])}
        print("%s: device wall %.2f ms (kernels %.3f ms, %d items downloaded, replay %.3f ms), host baseline %.2f ms, %.1f %% of the tracks selected"
              % (size, row["device_wall_ms_median"], row["device_kernel_ms_median"], r["deficient_items"], row["host_replay_ms_median"],
                 row["host_baseline_ms_median"], 100 * row["share_of_tracks_selected"]), flush=True)
        # the reference's 100 tracks per view leave no camera deficient on these scenes: a second setting that does, for the list and the replay
        kd = dict(kw, min_num_optimized_tracks_per_view=K_DEFICIENT)
        d = select_good_tracks(*args, **kd)
        dw, dk, dr = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            d = select_good_tracks(*args, **kd)
            dw.append(1e3 * (time.perf_counter() - t0)); dk.append(d["kernel_ms"]); dr.append(d["replay_ms"])
        t0 = time.perf_counter()
        hd = select_good_tracks_from_statistics(N, g["track_ptr"], g["obs_cam"], g["obs_xy"], d["n_views"], d["mean_sq_err"], **kd)
        row["deficient_setting"] = {"min_tracks_per_view": K_DEFICIENT, "device_wall_ms_median": float(np.median(dw)), "device_kernel_ms_median": float(np.median(dk)),
                                    "deficient_items": d["deficient_items"], "deficient_list_bytes": 12 * d["deficient_items"], "host_replay_ms_median": float(np.median(dr)),
                                    "host_replay_ms": dr, "host_baseline_ms": 1e3 * (time.perf_counter() - t0), "counts": d["counts"],
                                    "host_baseline_equals_device": bool(np.array_equal(hd["selected"], d["selected"]) and hd["counts"] == d["counts"])}
        print("  with %d tracks per view: device wall %.2f ms (kernels %.3f ms), %d items (%.1f MB) downloaded, host replay (sort and walk) %.2f ms, %d cameras topped up"
              % (K_DEFICIENT, np.median(dw), np.median(dk), d["deficient_items"], 12e-6 * d["deficient_items"], np.median(dr), d["counts"]["cameras_topped_up"]), flush=True)
        if not a.no_adjustment:
            for name, flags in (("all_tracks", None), ("selected_tracks", (r["selected"] != 0).astype(np.uint8))):
                P = FullBundleProblem(g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"], point_estimated=flags)
                P.set_loss(LF.HuberLoss(10.0))
                P.solve(w0, c0, p0, max_num_iterations=1)   # warm
                s = P.solve(w0, c0, p0)[3]
                P.close()
                row["adjustment_" + name] = {"solve_ms": s["t_total_ms"], "termination": s["termination_name"], "lm_iterations": s["num_iterations"],
                                             "pcg_iterations": s["num_cg_iterations"], "num_points": s["num_active_points"], "num_observations": s["num_observations_used"],
                                             "initial_cost": s["initial_cost"], "final_cost": s["final_cost"]}
                print("  gsfm_ba6_solve over %s: %.1f ms, %d LM / %d PCG iterations, %d points, %d observations"
                      % (name, s["t_total_ms"], s["num_iterations"], s["num_cg_iterations"], s["num_active_points"], s["num_observations_used"]), flush=True)
            row["adjustment_time_ratio_selected_over_all"] = row["adjustment_selected_tracks"]["solve_ms"] / row["adjustment_all_tracks"]["solve_ms"]
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
