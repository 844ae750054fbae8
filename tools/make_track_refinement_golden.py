#!/usr/bin/env python3
"""Writes tests/golden/track_refinement_spread.json: for every track of the refinement parity batch (tests/track_refinement_reference.py) the
50-digit result (status, point, iterations, termination, costs, whether a decision came within 1e-9 of its threshold) and the spread -- the
fp64 numpy restatement's worst relative deviation from the 50-digit point and final cost over 8 summation orders.  The device test allows
4 x spread_max.  CPU only; tests/test_track_refinement_reference.py recomputes the file's contents and checks them.  A "device_measured"
entry of the existing file (written by hand from a device run of tests/test_gpu_track_refinement.py) is carried over.

Then tests/golden/track_refinement_losses.json: the same fields for the sub-batch (ref.make_sub_batch: about sixty tracks picked by the first
file's iteration counts, plus hand-placed ones) under Tukey 10, Geman-McClure (10, 0.5) and SoftLOne 10."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import track_refinement_reference as ref  # noqa: E402


def main():
    doc = ref.compute_golden()
    path = os.path.join(ROOT, "tests", "golden", "track_refinement_spread.json")
    if os.path.exists(path):
        with open(path) as f:
            doc["device_measured"] = json.load(f).get("device_measured")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
    hist = {}
    for c in doc["cases"]:
        hist[c["status"]] = hist.get(c["status"], 0) + 1
    print("%d tracks, statuses %s, %d near a decision, spread_max %.3e -> %s" % (len(doc["cases"]), sorted(hist.items()), doc["num_near"],
                                                                                 doc["spread_max"], path))
    sub = ref.compute_sub_golden(ref.make_sub_batch(ref.make_batch(), doc["cases"]))
    path = os.path.join(ROOT, "tests", "golden", "track_refinement_losses.json")
    sub["device_measured"] = None
    if os.path.exists(path):
        with open(path) as f:
            sub["device_measured"] = json.load(f).get("device_measured")
    with open(path, "w") as f:
        json.dump(sub, f, indent=0)
    for name, d in sub["losses"].items():
        print("%s: %d tracks, %d near a decision, spread_max %.3e" % (name, len(d["cases"]), d["num_near"], d["spread_max"]))
    print("-> %s" % path)


if __name__ == "__main__":
    main()
