#!/usr/bin/env python3
"""Madrid Metropolis rotations two ways from the device's spanning-tree start: the robust L1 + IRLS estimator (Theia's ROBUST_L1L2) and
the nonlinear estimator with the MAGSAC loss, compared with each other in the manner of compare_orientations (the angles between the two
results after a rigid alignment)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from globalsfmpy_amd import _abi, solver, synth   # noqa: E402
from globalsfmpy_amd.loss_functions import MAGSACWeightBasedLoss   # noqa: E402

d = np.load(os.path.join(ROOT, "tests", "golden", "madrid_graph.npz"))
ids = np.sort(d["view_ids"])
ei, ej = np.searchsorted(ids, d["edge_a"]).astype(np.uint32), np.searchsorted(ids, d["edge_b"]).astype(np.uint32)
n, rel = ids.shape[0], np.ascontiguousarray(d["rel_aa"])

tree = solver.orientations_from_maximum_spanning_tree(n, ei, ej, rel, weight=None)
robust, s = solver.estimate_rotations_robust_l1l2(n, ei, ej, rel, tree["rot_aa"], fixed_cam=tree["root"])
print("ROBUST_L1L2: %d L1 iterations (ADMM %s), %d IRLS iterations, %d PCG iterations, %.1f ms"
      % (s["num_l1_iterations"], s["num_admm_iterations"], s["num_irls_iterations"], s["num_cg_iterations"], s["t_total_ms"]))

problem = solver.RotationProblem(n, ei, ej, rel, _abi.ANGLE_AXIS)
problem.set_loss(MAGSACWeightBasedLoss(0.02))
nonlinear, t = problem.solve(tree["rot_aa"])
print("NONLINEAR + MAGSAC(0.02): %d LM iterations, %.1f ms" % (t["num_iterations"], t["t_total_ms"]))

err = np.degrees(synth.angular_distance(synth.align_rotations(robust, nonlinear), nonlinear))
print("between the two, %d views: mean %.3f, median %.3f, max %.3f degrees; %d within 1 degree, %d within 5"
      % (n, err.mean(), np.median(err), err.max(), (err < 1.0).sum(), (err < 5.0).sum()))
