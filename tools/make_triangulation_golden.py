#!/usr/bin/env python3
"""Writes tests/golden/triangulation_spread.json: for every track of the triangulation parity batch (tests/triangulation_reference.py) the
50-digit result (status, point, the decisive quantities, whether one of them lies within 1e-9 of its threshold) and the spread -- the fp64
numpy restatement's worst deviation from the 50-digit point over 8 summation orders, relative to |X - centroid of the track's origins|.
The device test allows 4 x spread_max.  CPU only; tests/test_triangulation_reference.py recomputes the file's contents and checks them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import triangulation_reference as tri  # noqa: E402


def main():
    doc = tri.compute_golden()
    path = os.path.join(ROOT, "tests", "golden", "triangulation_spread.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
    hist = {}
    for c in doc["cases"]:
        hist[c["status"]] = hist.get(c["status"], 0) + 1
    print("%d tracks, statuses %s, %d near a threshold, spread_max %.3e -> %s" % (len(doc["cases"]), sorted(hist.items()), doc["num_near_threshold"],
                                                                                  doc["spread_max"], path))


if __name__ == "__main__":
    main()
