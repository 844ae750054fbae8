#!/usr/bin/env python3
"""Times gsfm_tracks_triangulate_refine (tracks triangulated, refined per track by Levenberg-Marquardt and gated in one launch per lane
class) on the scenes of tools/time_triangulation.py, about 1 M and 10 M observations.  Per size: warm median of --reps calls of the HIP-event
kernel time with and without the refinement (the latter is gsfm_tracks_triangulate on the same scene), the difference per
observation-iteration (an observation of a refined track counts once per iteration of that track, plus once for the pass at the midpoint),
the mean and maximum iterations, the status counts of both, and the numpy restatement's wall time on a sample of the same tracks scaled to
the scene by observation-iterations.  Writes profiles/track_refinement_times.json.
usage: tools/time_track_refinement.py [--reps 5] [--sizes 1M,10M] [--out profiles/track_refinement_times.json]"""
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

from globalsfmpy_amd import _abi, synth  # noqa: E402
from globalsfmpy_amd.solver import triangulate_tracks  # noqa: E402
import track_refinement_reference as ref  # noqa: E402
import triangulation_reference as tri  # noqa: E402
from time_triangulation import LENGTHS, MEAN_LENGTH, SIZES, WEIGHTS  # noqa: E402

HUBER10 = [(_abi.LOSS_HUBER, 10.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1M,10M")
    ap.add_argument("--numpy-sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_refinement_times.json"))
    a = ap.parse_args()
    rows = []
    for name in a.sizes.split(","):
        n_obs_target, n_cams = SIZES[name]
        g = synth.make_tracks(n_cams, int(round(n_obs_target / MEAN_LENGTH)), 31, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5, outlier_frac=0.02)
        T, n_obs = len(g["track_ptr"]) - 1, int(g["track_ptr"][-1])
        print("%s: %d tracks / %d observations / %d cameras" % (name, T, n_obs, n_cams), flush=True)
        args = (g["rot_aa"], g["cam_pos"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])
        kern = {False: [], True: []}
        for refine in (False, True):
            r = triangulate_tracks(*args, refine=refine, loss=HUBER10)   # warm-up
            for k in range(a.reps):
                r = triangulate_tracks(*args, refine=refine, loss=HUBER10)
                kern[refine].append(r["kernel_ms"])
            print("  refine=%s: kernel ms %s" % (refine, ["%.3f" % x for x in kern[refine]]), flush=True)
            if not refine:
                plain = r
        lengths = np.diff(g["track_ptr"].astype(np.int64))
        done = r["termination"] >= 0
        obs_iterations = int(np.sum(lengths[done] * (r["iterations"][done].astype(np.int64) + 1)))
        k0, k1 = float(np.median(kern[False])), float(np.median(kern[True]))
        good = r["status"] == 0
        row = {"name": name, "n_tracks": T, "n_obs": n_obs, "n_cams": n_cams, "reps": a.reps, "loss": "HUBER 10",
               "kernel_ms_unrefined_median": k0, "kernel_ms_refined_median": k1, "kernel_ms_unrefined": kern[False], "kernel_ms_refined": kern[True],
               "observation_iterations": obs_iterations, "refinement_ns_per_observation_iteration": 1e6 * (k1 - k0) / max(obs_iterations, 1),
               "mean_iterations": float(r["iterations"][done].mean()), "max_iterations": int(r["iterations"].max()),
               "status_counts_unrefined": [int(c) for c in plain["counts"]], "status_counts_refined": [int(c) for c in r["counts"]],
               "median_error_to_truth_unrefined": float(np.median(np.linalg.norm(plain["points"][plain["status"] == 0] - g["gt_points"][plain["status"] == 0], axis=1))),
               "median_error_to_truth_refined": float(np.median(np.linalg.norm(r["points"][good] - g["gt_points"][good], axis=1)))}
        # the numpy restatement on a sample of the same tracks, scaled by observation-iterations to the whole scene
        rng = np.random.Generator(np.random.PCG64(3))
        sample = rng.choice(T, size=min(a.numpy_sample, T), replace=False)
        ptr = g["track_ptr"].astype(np.int64)
        c, max_sq = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2
        t0 = time.perf_counter()
        agree = 0
        for t in sample:
            res = ref.refine_fp64(g, g["obs_cam"][ptr[t]:ptr[t + 1]], g["obs_xy"][ptr[t]:ptr[t + 1]], c, max_sq, order="lane")
            agree += int((res.status, res.iterations) == (r["status"][t], r["iterations"][t]))
        dt = time.perf_counter() - t0
        s_done = done[sample]
        s_oi = int(np.sum(lengths[sample][s_done] * (r["iterations"][sample][s_done].astype(np.int64) + 1)))
        row.update({"numpy_sample_tracks": int(sample.size), "numpy_sample_observation_iterations": s_oi, "numpy_sample_s": dt,
                    "numpy_scaled_to_scene_s": dt * obs_iterations / max(s_oi, 1), "numpy_sample_decision_agreement": agree})
        print(json.dumps({k: v for k, v in row.items() if not k.startswith("kernel_ms_") or k.endswith("median")}), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
