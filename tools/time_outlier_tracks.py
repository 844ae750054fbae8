#!/usr/bin/env python3
"""Times gsfm_tracks_outlier_tracks (the outlier rule after a bundle adjustment, a group of 4, 16 or 64 lanes per estimated track) on the two
scenes of tools/time_bundle_adjustment.py and tools/time_full_bundle_adjustment.py (synth.make_tracks, 500 cameras / 100 k tracks and 5 000 /
1 M; 0.5 px noise, 2 % gross outliers).  The points are the generator's plus those tools' 0.05 start offset: no solve is needed to time the
rule.  Per scene: warm median of --reps calls, wall time from host arrays and HIP-event kernel time; the kernel time with one lane class
estimated at a time (each of these spans k_tri_cameras too, which every call runs); the kernels' own byte count and
the fraction of the 8 TB/s stream floor on it, beside k_tri_tracks' on the same scene; and the wall time of the vectorised numpy restatement
below, with the number of tracks on which the two disagree.  Writes profiles/outlier_tracks_times.json.
usage: tools/time_outlier_tracks.py [--reps 5] [--sizes 500x100k,5000x1M] [--out profiles/outlier_tracks_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import synth  # noqa: E402
from globalsfmpy_amd.solver import outlier_tracks, triangulate_tracks  # noqa: E402
from time_bundle_adjustment import parse  # noqa: E402
from time_triangulation import HBM_BYTES_PER_S, LENGTHS, WEIGHTS, kernel_bytes as triangulation_bytes  # noqa: E402
import triangulation_reference as tri  # noqa: E402

MAX_ERR_PX, MIN_ANGLE_DEG = 5.0, 4.0


def kernel_bytes(lengths, n_cams):
    """what the track kernels must move: per observation the 4 B camera index read by the ray pass and again, with the 16 B pixel, by the gate;
    per observation of a track of 65 or more the 24 B ray written and read back; per track 16 B of offsets and order, the 24 B point and
    16 B of outputs.  The 128 B camera records are gathered from cache and counted once."""
    n_obs = int(lengths.sum())
    long_obs = int(lengths[lengths > tri.LEN_G16].sum())
    return 24 * n_obs + 48 * long_obs + 56 * len(lengths) + 128 * n_cams


def outlier_numpy(g, points, max_err=MAX_ERR_PX, min_angle=MIN_ANGLE_DEG, chunk_elems=1 << 24):
    """the rule of include/gsfm_tracks.h vectorised over observations (every camera and track estimated); the pair cosines per group of
    tracks of one length, in chunks"""
    ptr = g["track_ptr"].astype(np.int64)
    lengths = np.diff(ptr)
    T = len(lengths)
    track = np.repeat(np.arange(T), lengths)
    cam = g["obs_cam"]
    R = synth.aa_to_matrix(g["rot_aa"])
    w = points[track] - g["cam_pos"][cam]
    with np.errstate(all="ignore"):
        p = np.einsum("eij,ej->ei", R[cam], w)
        K = g["intrinsics"][cam]
        e = K[:, :1] * p[:, :2] / p[:, 2:] + K[:, 1:] - g["obs_xy"]
        mean = np.bincount(track, weights=(e * e).sum(axis=1), minlength=T) / lengths
        behind = np.bincount(track, weights=p[:, 2] < 0, minlength=T) > 0
        d = w / np.sqrt((w * w).sum(axis=1))[:, None]
    c = np.cos(np.radians(min_angle))
    wide = np.zeros(T, dtype=bool)
    for L in np.unique(lengths):
        if L < 2:
            continue
        ts = np.flatnonzero(lengths == L)
        iu = np.triu_indices(L, 1)
        step = max(1, chunk_elems // (L * L))
        for k in range(0, len(ts), step):
            sel = ts[k:k + step]
            D = d[(ptr[sel][:, None] + np.arange(L)[None, :]).reshape(-1)].reshape(len(sel), L, 3)
            G = D @ D.transpose(0, 2, 1)
            wide[sel] = (G[:, iu[0], iu[1]] < c).any(axis=1)
    return np.where(behind, 2, np.where(mean > max_err * max_err, 3, np.where(wide, 0, 4))).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x100k,5000x1M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_tracks_times.json"))
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        n_cams, n_tracks = parse(size)
        t0 = time.perf_counter()
        g = synth.make_tracks(n_cams, n_tracks, 31, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5, outlier_frac=0.02)
        N, T, O = n_cams, n_tracks, int(g["track_ptr"][-1])
        rng = np.random.default_rng(1)
        rng.standard_normal((N, 3))                                   # the bundle-adjustment tools draw the centres' offsets first
        points = g["gt_points"] + 0.05 * rng.standard_normal((T, 3))
        lengths = np.diff(g["track_ptr"].astype(np.int64))
        print("%s: %d tracks / %d observations / %d cameras generated in %.1f s" % (size, T, O, N, time.perf_counter() - t0), flush=True)
        args = (g["rot_aa"], g["cam_pos"], g["intrinsics"], g["track_ptr"], g["obs_cam"], g["obs_xy"], points)
        kw = dict(max_reprojection_error_pixels=MAX_ERR_PX, min_triangulation_angle_degrees=MIN_ANGLE_DEG)

        def timed(**more):
            r = outlier_tracks(*args, **kw, **more)   # warm-up
            wall, kern = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = outlier_tracks(*args, **kw, **more)
                wall.append(1e3 * (time.perf_counter() - t0)); kern.append(r["kernel_ms"])
            return r, wall, kern
        r, wall, kern = timed()
        nbytes = kernel_bytes(lengths, N)
        kms = float(np.median(kern))
        row = {"name": size, "n_tracks": T, "n_obs": O, "n_cams": N, "reps": a.reps, "wall_ms_median": float(np.median(wall)), "kernel_ms_median": kms,
               "wall_ms": wall, "kernel_ms": kern, "kernel_ns_per_observation": 1e6 * kms / O, "kernel_bytes": nbytes, "bytes_per_observation": nbytes / O,
               "stream_floor_ms": 1e3 * nbytes / HBM_BYTES_PER_S, "fraction_of_stream_floor": (1e3 * nbytes / HBM_BYTES_PER_S) / kms,
               "status_counts": [int(c) for c in r["counts"]], "classes": {}}
        print("  all classes: wall %.1f ms, kernel %.3f ms, %.1f %% of the stream floor" % (row["wall_ms_median"], kms, 100 * row["fraction_of_stream_floor"]), flush=True)
        cls = np.array([tri.lane_class(x) for x in lengths])
        for G in (4, 16, 64):
            sel = cls == G
            _, _, kc = timed(point_estimated=sel)
            cb = kernel_bytes(lengths[sel], N)
            us = 1e3 * float(np.median(kc))
            row["classes"][str(G)] = {"n_tracks": int(sel.sum()), "n_obs": int(lengths[sel].sum()), "kernel_us_median_with_camera_kernel": us,
                                      "kernel_us": [1e3 * x for x in kc], "kernel_bytes": cb, "fraction_of_stream_floor": (1e6 * cb / HBM_BYTES_PER_S) / us}
            print("  class %2d: %d tracks, %d observations, kernel %.1f us (with k_tri_cameras)" % (G, sel.sum(), lengths[sel].sum(), us), flush=True)
        # k_tri_tracks on the same scene, per byte of its own model
        t3 = triangulate_tracks(*args[:6])
        kt = []
        for _ in range(a.reps):
            t3 = triangulate_tracks(*args[:6])
            kt.append(t3["kernel_ms"])
        tb = triangulation_bytes(g, t3["status"])
        row["triangulation"] = {"kernel_ms_median": float(np.median(kt)), "kernel_bytes": tb,
                                "fraction_of_stream_floor": (1e3 * tb / HBM_BYTES_PER_S) / float(np.median(kt))}
        # the vectorised numpy restatement on the same host
        t0 = time.perf_counter()
        ref = outlier_numpy(g, points)
        row["numpy_s"] = time.perf_counter() - t0
        row["numpy_status_disagreements"] = int((ref != r["status"]).sum())
        print(json.dumps({k: v for k, v in row.items() if k not in ("wall_ms", "kernel_ms")}), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
