#!/usr/bin/env python3
"""Camera-position estimation at benchmark scale: make_position_graph on the rotation benchmark's edge set (100k cameras, 10M edges,
seed 2023), 30 % outlier directions, HuberLoss(0.1), the all-zero start, camera 0 fixed.  Prints one JSON line.

  python tools/bench_positions.py [--cams N --edges E --steps K --warmup W]          ms per solve, LM and PCG iteration counts
  rocprofv3 --kernel-trace --stats -d DIR -o pos -- python tools/bench_positions.py --steps 1 --warmup 0
  python tools/bench_positions.py --stats DIR/pos_results.db --timing LINE.json   (or the kernel_stats.csv of a CSV-format run)
        (no GPU) the timing line merged with the per-kernel times of the profiled run, each kernel's byte model and its fraction of
        8 TB/s.  Byte models count every array element once and a gathered camera as 24 B (cache-line over-fetch not counted).
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12


def byte_models(N, E):
    nd = 2 * E
    return {
        # per entry: neighbour 4, signed direction 24, gathered x_m 24, H_e written 48; per row: row_ptr 4, x_k 24, g 24, D_k 48
        "k_pos_lin": nd * (4 + 24 + 24 + 48) + N * (4 + 24 + 24 + 48),
        # per entry: neighbour 4, H_e 48, gathered q_m 24; per row: row_ptr 4, active 1, q p S D2 96, out 24
        "k_pos_matvec": nd * (4 + 48 + 24) + N * (4 + 1 + 96 + 24),
        # per edge: i, j 8, direction 24, two gathered positions 48
        "k_pos_cost": E * (8 + 24 + 48),
    }


def merge(stats_path, timing):
    N, E = timing["n_cams"], timing["n_edges"]
    models = byte_models(N, E)
    if stats_path.endswith(".db"):   # rocprofv3's default output: the `kernels` view of its SQLite database
        import sqlite3
        con = sqlite3.connect(stats_path)
        rows = [{"Name": n, "Calls": c, "TotalDurationNs": t} for n, c, t in con.execute("select name, count(*), sum(end - start) from kernels group by name")]
    else:
        rows = list(csv.DictReader(open(stats_path)))
    out = {}
    for key in models:
        hit = [r for r in rows if key in r["Name"] and (key != "k_pos_matvec" or "true" in r["Name"] or "(bool)1" in r["Name"])]
        if not hit:
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        total_ns = sum(float(r["TotalDurationNs"]) for r in hit)
        us = total_ns / calls / 1e3
        out[key] = {"calls": calls, "us_per_call": round(us, 2), "bytes_per_call": models[key],
                    "frac_of_8TBps": round(models[key] / (us * 1e-6) / HBM, 3)}
    timing = dict(timing)
    timing["kernels"] = out
    return timing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=100000)
    ap.add_argument("--edges", type=int, default=10000000)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stats", help="rocprofv3 results .db or kernel_stats.csv of a profiled run (merge mode, no GPU)")
    ap.add_argument("--timing", help="the JSON line of a plain run (merge mode)")
    args = ap.parse_args()
    if args.stats:
        timing = json.loads(open(args.timing).read().strip().splitlines()[-1])
        print(json.dumps(merge(args.stats, timing)))
        return
    from globalsfmpy_amd import synth
    from globalsfmpy_amd import loss_functions as lf
    from globalsfmpy_amd.solver import PositionProblem
    t0 = time.time()
    g = synth.make_position_graph(args.cams, args.edges, args.seed, outlier_frac=args.outliers, noise=args.noise)
    t_gen = time.time() - t0
    t0 = time.time()
    p = PositionProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"])
    p.set_loss(lf.HuberLoss(0.1))
    t_create = time.time() - t0
    ms, s = [], None
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        x, s = p.solve(None, fixed_cam=0)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            ms.append(dt)
    ms.sort()
    print(json.dumps({"metric": "position_solve_ms", "n_cams": args.cams, "n_edges": int(g["edge_i"].size), "outliers": args.outliers,
                      "loss": "HuberLoss(0.1)", "ms_per_solve": round(ms[len(ms) // 2], 2), "ms_all": [round(v, 2) for v in ms],
                      "lm_iterations": s["num_iterations"], "successful_steps": s["num_successful_steps"],
                      "pcg_iterations": s["num_cg_iterations"], "pcg_stalled_steps": s["num_pcg_stalled_steps"],
                      "termination": s["termination_name"], "initial_cost": s["initial_cost"], "final_cost": s["final_cost"],
                      "create_s": round(t_create, 2), "generate_s": round(t_gen, 2)}))


if __name__ == "__main__":
    main()
