"""Writes tests/golden/robust_rotation_spread.json: how far the fp64 restatement of the robust L1 + IRLS rotation estimator
(tests/robust_rotation_reference.py) is from a better answer, on the inputs of tests/test_gpu_robust_rotations.py.  The device is held to
4 x these figures.
  residual            the largest deviation of the fp64 residuals from an mpmath evaluation (50 digits) over the edges of residual_case()
  madrid              the largest deviation of the linear="pcg" restatement's rotations from the linear="direct" ones on Madrid, at the
                      library's default cg_relative_tolerance; with the stage counts of both
  laplacian_weighted / laplacian_unit
                      the largest deviation of the restatement's PCG solution from the dense solution on laplacian_case(), with the PCG's
                      iteration count
  madrid_by_tolerance the same Madrid deviation and the PCG iterations at other tolerances (the table of DESIGN.md, section 23)
Run from the repository root:  python tests/golden/make_robust_rotation_spread.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import robust_rotation_cases as cases   # noqa: E402
import robust_rotation_reference as ref   # noqa: E402

OUT = os.path.join(HERE, "robust_rotation_spread.json")


def compute(with_table=True):
    spread = {}
    c = cases.residual_case()
    spread["residual"] = float(np.abs(ref.residuals(c["edge_i"], c["edge_j"], c["rel_aa"], c["rot_aa"]) - cases.mp_residuals(c)).max())
    m, rot_direct, log_direct = cases.solved("madrid")

    def madrid_pcg(tol):
        rot, log = ref.solve(m["n_cams"], m["edge_i"], m["edge_j"], m["rel_aa"], m["init_aa"], m["fixed_cam"], linear="pcg", cg_relative_tolerance=tol)
        return float(np.abs(rot - rot_direct).max()), log
    dev, log = madrid_pcg(ref.DEFAULTS["cg_relative_tolerance"])
    spread["madrid"] = {"deviation": dev, "cg_relative_tolerance": ref.DEFAULTS["cg_relative_tolerance"], "admm_iterations": log["admm_iterations"],
                        "irls_iterations": log["irls_iterations"], "direct_admm_iterations": log_direct["admm_iterations"],
                        "direct_irls_iterations": log_direct["irls_iterations"], "cg_iterations": log["cg_iterations"]}
    lc = cases.laplacian_case()
    for name, w in (("laplacian_weighted", lc["weights"]), ("laplacian_unit", None)):
        dense, _, _ = ref.laplacian_solve(lc["n_cams"], lc["edge_i"], lc["edge_j"], lc["rhs"], w, lc["fixed_cam"], linear="dense")
        x, it, rel = ref.laplacian_solve(lc["n_cams"], lc["edge_i"], lc["edge_j"], lc["rhs"], w, lc["fixed_cam"], linear="pcg")
        spread[name] = {"deviation": float(np.abs(x - dense).max()), "cg_iterations": int(it), "scale": float(np.abs(dense).max())}
    if with_table:
        spread["madrid_by_tolerance"] = []
        for tol in (1e-10, 1e-12, 1e-14, 1e-15):
            d, lg = madrid_pcg(tol)
            spread["madrid_by_tolerance"].append({"cg_relative_tolerance": tol, "deviation": d, "cg_iterations": lg["cg_iterations"]})
    return spread


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(compute(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(OUT).read())
