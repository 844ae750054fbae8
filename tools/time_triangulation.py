#!/usr/bin/env python3
"""Times gsfm_tracks_triangulate (tracks triangulated by the midpoint method and gated, a group of 4, 16 or 64 lanes per track) on
synth.make_tracks scenes of about 1 M and 10 M observations with a 1DSfM-like mix of track lengths (most tracks shorter than 8, a tail up
to 1000).  Per size: warm median of --reps calls, wall time and HIP-event kernel time, nanoseconds per observation, the kernel's own byte
count and the fraction of the 8 TB/s stream floor on it, and the numpy restatement's wall time on a sample of the
same tracks scaled to the scene by observations, printed beside the kernel time.  Writes profiles/triangulation_times.json.
usage: tools/time_triangulation.py [--reps 5] [--sizes 1M,10M] [--out profiles/triangulation_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import synth  # noqa: E402
from globalsfmpy_amd.solver import triangulate_tracks  # noqa: E402
import triangulation_reference as tri  # noqa: E402

LENGTHS = (2, 3, 4, 5, 6, 7, 8, 10, 13, 20, 35, 64, 65, 120, 300, 1000)
WEIGHTS = (0.42, 0.2, 0.11, 0.07, 0.05, 0.035, 0.025, 0.03, 0.02, 0.015, 0.01, 0.005, 0.004, 0.003, 0.0025, 0.0005)
MEAN_LENGTH = float(np.dot(LENGTHS, WEIGHTS))
SIZES = {"1M": (1000000, 2000), "10M": (10000000, 5000)}      # observations aimed at, cameras
HBM_BYTES_PER_S = 8e12


def kernel_bytes(g, status):
    """what the track kernels must move: per observation the 4 B camera index and the 16 B pixel, read in pass 1 and again by the gate of
    the tracks that reach it; per observation of a track of 65 or more the 24 B ray written and read back; per track 16 B of offsets and
    order and 40 B of outputs.  The 128 B camera records (n_cams x 128 B) are gathered from cache and counted once."""
    lengths = np.diff(g["track_ptr"].astype(np.int64))
    n_obs = int(lengths.sum())
    gated = int(lengths[np.isin(status, (0, 4, 5))].sum())
    long_obs = int(lengths[lengths > tri.LEN_G16].sum())
    return 20 * (n_obs + gated) + 48 * long_obs + 56 * len(lengths) + 128 * g["n_cams"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1M,10M")
    ap.add_argument("--numpy-sample", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulation_times.json"))
    a = ap.parse_args()
    rows = []
    for name in a.sizes.split(","):
        n_obs_target, n_cams = SIZES[name]
        t0 = time.perf_counter()
        g = synth.make_tracks(n_cams, int(round(n_obs_target / MEAN_LENGTH)), 31, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5, outlier_frac=0.02)
        T, n_obs = len(g["track_ptr"]) - 1, int(g["track_ptr"][-1])
        print("%s: %d tracks / %d observations / %d cameras generated in %.1f s" % (name, T, n_obs, n_cams, time.perf_counter() - t0), flush=True)
        args = (g["rot_aa"], g["cam_pos"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"])
        r = triangulate_tracks(*args)   # warm-up
        wall, kern = [], []
        for k in range(a.reps):
            t0 = time.perf_counter()
            r = triangulate_tracks(*args)
            wall.append(1e3 * (time.perf_counter() - t0)); kern.append(r["kernel_ms"])
            print("  call %d: wall %.1f ms, kernel %.3f ms" % (k, wall[-1], kern[-1]), flush=True)
        nbytes = kernel_bytes(g, r["status"])
        kms = float(np.median(kern))
        good = r["status"] == 0
        row = {"name": name, "n_tracks": T, "n_obs": n_obs, "n_cams": n_cams, "reps": a.reps, "wall_ms_median": float(np.median(wall)),
               "kernel_ms_median": kms, "wall_ms": wall, "kernel_ms": kern, "kernel_ns_per_observation": 1e6 * kms / n_obs,
               "kernel_bytes": nbytes, "bytes_per_observation": nbytes / n_obs, "stream_floor_ms": 1e3 * nbytes / HBM_BYTES_PER_S,
               "fraction_of_stream_floor": (1e3 * nbytes / HBM_BYTES_PER_S) / kms, "status_counts": [int(c) for c in r["counts"]],
               "median_error_to_truth": float(np.median(np.linalg.norm(r["points"][good] - g["gt_points"][good], axis=1)))}
        # the numpy restatement on a sample of the same tracks, scaled by observations to the whole scene
        rng = np.random.Generator(np.random.PCG64(3))
        sample = rng.choice(T, size=min(a.numpy_sample, T), replace=False)
        ptr = g["track_ptr"].astype(np.int64)
        c, max_sq = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2
        t0 = time.perf_counter()
        agree = 0
        for t in sample:
            res = tri.triangulate_fp64(g, g["obs_cam"][ptr[t]:ptr[t + 1]], g["obs_xy"][ptr[t]:ptr[t + 1]], c, max_sq)
            agree += int(res.status == r["status"][t])
        dt = time.perf_counter() - t0
        sobs = int(np.sum(ptr[sample + 1] - ptr[sample]))
        row.update({"numpy_sample_tracks": int(sample.size), "numpy_sample_observations": sobs, "numpy_sample_s": dt,
                    "numpy_scaled_to_scene_s": dt * n_obs / sobs, "numpy_sample_status_agreement": agree})
        print(json.dumps({k: v for k, v in row.items() if k not in ("wall_ms", "kernel_ms")}), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
