#!/usr/bin/env python3
"""Times gsfm_pos_refine_relative_translations (relative translations refined with known rotations, one wavefront per view pair) at two
sizes: Madrid's 23 784 edges with match counts drawn as synth.spanning_tree_init draws them (150-1500 for 70 % of the edges, 16-150 for
the rest, whose second-view points are mismatched), and one large synthetic batch (100 000 edges of 16-400 matches).  Per size: warm median
of --reps calls, wall time and HIP-event kernel time, nanoseconds per match and IRLS iteration, and the numpy restatement's wall time on a
sample of the same edges scaled to the batch, printed beside the kernel time.  Writes profiles/translation_refinement_times.json.
usage: tools/time_translation_refinement.py [--reps 5] [--sizes madrid,large] [--out profiles/translation_refinement_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd.solver import refine_relative_translations  # noqa: E402
import translation_refinement_reference as trr  # noqa: E402

SIZES = {"madrid": (23784, (150, 1500), (16, 150), 0.3), "large": (100000, (16, 400), (16, 400), 0.0)}


def rodrigues(w):
    th = np.linalg.norm(w, axis=1)[:, None, None]
    k = w / th[:, :, 0]
    Kx = np.zeros((w.shape[0], 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def make_batch(n_edges, inlier_matches, outlier_matches, outlier_frac, seed=21, noise_px=0.5):
    """vectorised two-view pairs (the geometry of covariance.make_two_view_batch): every edge has its own two cameras, camera i at the
    identity, camera j at the relative rotation; an outlier edge has few matches and 30 % of them mismatched"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = rng.random(n_edges) < outlier_frac
    counts = rng.integers(inlier_matches[0], inlier_matches[1], n_edges)
    counts[out] = rng.integers(outlier_matches[0], outlier_matches[1], int(out.sum()))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    M = int(ptr[-1])
    edge = np.repeat(np.arange(n_edges), counts)
    f = rng.uniform(800, 1600, (n_edges, 2))
    pp = rng.uniform(300, 900, (n_edges, 4))
    w = rng.uniform(-0.4, 0.4, (n_edges, 3))
    R = rodrigues(w)
    t = rng.standard_normal((n_edges, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    X1 = np.c_[rng.uniform(-2, 2, M), rng.uniform(-1.5, 1.5, M), rng.uniform(4, 9, M)]
    X2 = np.einsum("mrc,mc->mr", R[edge], X1 + t[edge])
    x1 = f[edge, :1] * X1[:, :2] / X1[:, 2:] + pp[edge, :2] + noise_px * rng.standard_normal((M, 2))
    x2 = f[edge, 1:] * X2[:, :2] / X2[:, 2:] + pp[edge, 2:] + noise_px * rng.standard_normal((M, 2))
    bad = out[edge] & (rng.random(M) < 0.3)
    x2[bad] = rng.uniform(0.0, 1200.0, (int(bad.sum()), 2))
    rot = np.zeros((2 * n_edges, 3))
    rot[1::2] = w
    return {"n_cams": 2 * n_edges, "edge_i": np.arange(0, 2 * n_edges, 2, dtype=np.uint32), "edge_j": np.arange(1, 2 * n_edges, 2, dtype=np.uint32),
            "match_ptr": ptr, "matches": np.ascontiguousarray(np.c_[x1, x2]), "intrinsics": np.c_[f[:, 0], pp[:, :2], f[:, 1], pp[:, 2:]],
            "rot_aa": rot, "rel_t": -t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="madrid,large")
    ap.add_argument("--numpy-sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translation_refinement_times.json"))
    a = ap.parse_args()
    rows = []
    for name in a.sizes.split(","):
        n_edges, inl, outl, frac = SIZES[name]
        t0 = time.perf_counter()
        b = make_batch(n_edges, inl, outl, frac)
        M = int(b["match_ptr"][-1])
        print("%s: %d edges / %d matches generated in %.1f s" % (name, n_edges, M, time.perf_counter() - t0), flush=True)
        args = (b["n_cams"], b["edge_i"], b["edge_j"], b["match_ptr"], b["matches"], b["intrinsics"], b["rot_aa"], b["rel_t"])
        out, info = refine_relative_translations(*args)   # warm-up
        wall, kern = [], []
        for r in range(a.reps):
            t0 = time.perf_counter()
            out, info = refine_relative_translations(*args)
            wall.append(1e3 * (time.perf_counter() - t0)); kern.append(info["kernel_ms"])
            print("  call %d: wall %.1f ms, kernel %.2f ms" % (r, wall[-1], kern[-1]), flush=True)
        counts = np.diff(b["match_ptr"].astype(np.int64))
        work = float(np.sum(counts * info["iterations"]))          # match-iterations
        cos = np.abs(np.sum(out * b["rel_t"], axis=1))
        row = {"name": name, "n_edges": n_edges, "n_matches": M, "reps": a.reps, "wall_ms_median": float(np.median(wall)),
               "kernel_ms_median": float(np.median(kern)), "wall_ms": wall, "kernel_ms": kern,
               "iterations_mean": float(info["iterations"].mean()), "iterations_max": int(info["iterations"].max()),
               "match_iterations": work, "kernel_ns_per_match_iteration": float(1e6 * np.median(kern) / work),
               "status_counts": [int((info["status"] == s).sum()) for s in range(3)],
               "median_angle_to_truth_rad": float(np.median(np.arccos(np.clip(cos, 0, 1))))}
        # the numpy restatement on a sample of the same edges, scaled by match-iterations to the whole batch
        rng = np.random.Generator(np.random.PCG64(3))
        sample = rng.choice(n_edges, size=min(a.numpy_sample, n_edges), replace=False)
        t0 = time.perf_counter()
        swork = 0.0
        for e in sample:
            lo, hi = int(b["match_ptr"][e]), int(b["match_ptr"][e + 1])
            r = trr.refine_fp64(b["matches"][lo:hi], b["intrinsics"][e], b["rot_aa"][2 * e], b["rot_aa"][2 * e + 1])
            swork += (hi - lo) * r.iterations
        dt = time.perf_counter() - t0
        row["numpy_sample_edges"] = int(sample.size)
        row["numpy_sample_s"] = dt
        row["numpy_scaled_to_batch_s"] = dt * work / swork
        print(json.dumps({k: v for k, v in row.items() if k not in ("wall_ms", "kernel_ms")}), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
