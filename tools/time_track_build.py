#!/usr/bin/env python3
"""Times gsfm_tracks_build (tracks from two-view matches on the device: Theia's TrackBuilder under the definition of include/gsfm_tracks.h)
on a synthetic scene of about 5 000 views and 20 M matches: synth.make_tracks' points seen by 2 to 8 views each, every pair of a track's
observations one match of that view pair, the matches flattened by sorted view pair as the COLMAP ingestion flattens them.  Warm median of
--reps calls: HIP-event kernel time and whole-call wall time (uploads, the host's looks at the component rounds, downloads), beside the
wall time of gsfm_tracks_build_sequential -- the C++ sequential restatement, one host thread -- on the same arrays; both results are
compared byte for byte.  Writes profiles/track_build_times.json.
usage: tools/time_track_build.py [--matches 20000000] [--views 5000] [--reps 3] [--out profiles/track_build_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from globalsfmpy_amd import synth  # noqa: E402
from globalsfmpy_amd.solver import build_tracks  # noqa: E402

LENGTHS = (2, 3, 4, 5, 6, 8)
WEIGHTS = (0.42, 0.2, 0.12, 0.1, 0.08, 0.08)
MATCHES_PER_TRACK = float(sum(w * n * (n - 1) / 2 for n, w in zip(LENGTHS, WEIGHTS)))


def make_matches(n_views, n_matches, seed):
    """(edge_i, edge_j, match_ptr, matches, n_tracks): all pairs of every track's observations, grouped by view pair (smaller view first)"""
    g = synth.make_tracks(n_views, int(round(n_matches / MATCHES_PER_TRACK)), seed, lengths=LENGTHS, length_weights=WEIGHTS, noise_px=0.5)
    ptr = g["track_ptr"].astype(np.int64)
    length = np.diff(ptr)
    first, second = [], []
    for n in LENGTHS:
        a, b = np.triu_indices(n, 1)
        start = ptr[:-1][length == n]
        first.append((start[:, None] + a[None, :]).reshape(-1)); second.append((start[:, None] + b[None, :]).reshape(-1))
    first, second = np.concatenate(first), np.concatenate(second)
    va, vb = g["obs_cam"][first].astype(np.int64), g["obs_cam"][second].astype(np.int64)
    swap = va > vb
    first, second = np.where(swap, second, first), np.where(swap, first, second)
    va, vb = np.minimum(va, vb), np.maximum(va, vb)
    key = va * n_views + vb
    order = np.argsort(key, kind="stable")
    key, first, second = key[order], first[order], second[order]
    edges, counts = np.unique(key, return_counts=True)
    match_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    matches = np.ascontiguousarray(np.concatenate([g["obs_xy"][first], g["obs_xy"][second]], axis=1))
    return (edges // n_views).astype(np.uint32), (edges % n_views).astype(np.uint32), match_ptr, matches, len(length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=20000000)
    ap.add_argument("--views", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_build_times.json"))
    a = ap.parse_args()
    t0 = time.perf_counter()
    edge_i, edge_j, match_ptr, matches, n_points = make_matches(a.views, a.matches, 31)
    M = int(match_ptr[-1])
    print("%d matches on %d view pairs of %d views (%d points) generated in %.1f s" % (M, len(edge_i), a.views, n_points, time.perf_counter() - t0), flush=True)
    args = (a.views, edge_i, edge_j, match_ptr, matches)
    r = build_tracks(*args)   # warm-up
    wall, kern = [], []
    for k in range(a.reps):
        t0 = time.perf_counter()
        r = build_tracks(*args)
        wall.append(1e3 * (time.perf_counter() - t0)); kern.append(r["kernel_ms"])
        print("  device call %d: wall %.1f ms, kernel %.3f ms" % (k, wall[-1], kern[-1]), flush=True)
    t0 = time.perf_counter()
    s = build_tracks(*args, sequential=True)
    seq_ms = 1e3 * (time.perf_counter() - t0)
    print("  sequential C++: wall %.1f ms" % seq_ms, flush=True)
    same = (r["counts"] == s["counts"] and r["track_ptr"].tobytes() == s["track_ptr"].tobytes() and r["obs_view"].tobytes() == s["obs_view"].tobytes()
            and r["obs_xy"].tobytes() == s["obs_xy"].tobytes())
    row = {"n_views": a.views, "n_edges": int(len(edge_i)), "n_matches": M, "n_points": n_points, "reps": a.reps, "counts": r["counts"],
           "n_observations": int(r["track_ptr"][-1]), "kernel_ms_median": float(np.median(kern)), "wall_ms_median": float(np.median(wall)),
           "kernel_ms": kern, "wall_ms": wall, "kernel_ns_per_match": 1e6 * float(np.median(kern)) / M, "sequential_cpp_wall_ms": seq_ms,
           "device_equals_sequential": bool(same)}
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
    if not same:
        sys.exit("the device result differs from the sequential restatement")


if __name__ == "__main__":
    main()
