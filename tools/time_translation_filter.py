#!/usr/bin/env python3
"""Times gsfm_pos_filter_relative_translations (the 1DSfM relative-translation filter) on synthetic graphs of the sizes that matter:
Madrid's 394 cameras / 23 784 edges, a Trafalgar-sized 5 288-camera graph, 10 k / 200 k and the benchmark's 100 k / 10 M (proj_out = NULL
everywhere).  Per size: warm median of --reps calls, wall time and HIP-event kernel time, passes and score picks per projection, and the
numpy restatement's time where one projection's time says it finishes in a minute.  Writes profiles/translation_filter_times.json.
usage: tools/time_translation_filter.py [--reps 7] [--sizes madrid,trafalgar,10k,100k] [--out profiles/translation_filter_times.json]"""
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
from globalsfmpy_amd.solver import filter_relative_translations  # noqa: E402
import translation_filter_reference as tfr  # noqa: E402

SIZES = {"madrid": (394, 23784), "trafalgar": (5288, 680000), "10k": (10000, 200000), "100k": (100000, 10000000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="madrid,trafalgar,10k,100k")
    ap.add_argument("--projections", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translation_filter_times.json"))
    a = ap.parse_args()
    rows = []
    for name in a.sizes.split(","):
        n_cams, n_edges = SIZES[name]
        t0 = time.perf_counter()
        g = synth.make_position_graph(n_cams, n_edges, seed=21, outlier_frac=0.3, noise=0.01)
        print("%s: %d cameras / %d edges generated in %.1f s" % (name, n_cams, len(g["edge_i"]), time.perf_counter() - t0), flush=True)
        args = (g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"])
        keep, out = filter_relative_translations(*args, num_iterations=a.projections, tolerance=0.08)   # warm-up
        wall, kern = [], []
        for r in range(a.reps):
            t0 = time.perf_counter()
            keep, out = filter_relative_translations(*args, num_iterations=a.projections, tolerance=0.08)
            wall.append(1e3 * (time.perf_counter() - t0)); kern.append(out["kernel_ms"])
            print("  call %d: wall %.1f ms, kernels %.1f ms" % (r, wall[-1], kern[-1]), flush=True)
        row = {"name": name, "n_cams": n_cams, "n_edges": int(len(g["edge_i"])), "projections": a.projections, "reps": a.reps,
               "wall_ms_median": float(np.median(wall)), "kernel_ms_median": float(np.median(kern)), "wall_ms": wall, "kernel_ms": kern,
               "n_kept": out["n_kept"], "passes_mean": float(out["num_passes"].mean()), "passes_max": int(out["num_passes"].max()),
               "picks_mean": float(out["num_picks"].mean()),
               "kernel_us_per_pass": float(1e3 * np.median(kern) / max(1, int(out["num_passes"].max())))}
        # the numpy restatement on the same axes: one projection first, all of them when that says a minute is enough
        if n_edges <= 1000000:
            d = tfr.world_directions(g["edge_i"], g["rel_t"], g["rot_aa"])
            proj = d @ out["axes"].T
            t0 = time.perf_counter()
            tfr.filter_from_projections(g["n_cams"], g["edge_i"], g["edge_j"], proj[:, :1], 0.08)
            one = time.perf_counter() - t0
            row["numpy_one_projection_s"] = one
            if one * a.projections < 60.0:
                t0 = time.perf_counter()
                tfr.filter_from_projections(g["n_cams"], g["edge_i"], g["edge_j"], proj, 0.08)
                row["numpy_s"] = time.perf_counter() - t0
        print(json.dumps({k: v for k, v in row.items() if k not in ("wall_ms", "kernel_ms")}), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
