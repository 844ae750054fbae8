"""The robust L1 + IRLS rotation estimator on the device (include/gsfm_rot_l1l2.h) against the numpy / scipy restatement of its
definition (tests/robust_rotation_reference.py, linear="direct").  The inputs are those of tests/robust_rotation_cases.py, whose decision
margins tests/test_robust_rotation_reference.py checks: both sides take the same decisions, so the stage counts are compared exactly."""
import json
import os

import numpy as np
import pytest

from globalsfmpy_amd import solver

import robust_rotation_cases as cases
import robust_rotation_reference as ref

pytestmark = pytest.mark.gpu

with open(os.path.join(cases.GOLDEN, "robust_rotation_spread.json")) as _f:
    SPREAD = json.load(_f)


def device_solve(c, **options):
    return solver.estimate_rotations_robust_l1l2(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["init_aa"], c["fixed_cam"], **options)


def assert_same_run(summary, log, rot, rot_ref, rot_tol, steps=True):
    print("device: admm %s l1 steps %s irls %d last step %.6e cg %d stalled %d worst cg residual %.3e | max |rot - ref| %.3e rad (bound %.1e)"
          % (summary["num_admm_iterations"], ["%.9e" % v for v in summary["l1_step"]], summary["num_irls_iterations"], summary["last_irls_step"],
             summary["num_cg_iterations"], summary["num_pcg_stalled_solves"], summary["worst_accepted_cg_residual"], np.abs(rot - rot_ref).max(), rot_tol))
    assert summary["nonfinite"] == 0
    assert summary["num_l1_iterations"] == len(log["admm_iterations"])
    assert summary["num_admm_iterations"] == log["admm_iterations"]
    assert summary["num_irls_iterations"] == log["irls_iterations"]
    assert bool(summary["l1_converged"]) == log["l1_converged"] and bool(summary["irls_converged"]) == log["irls_converged"]
    if steps:
        np.testing.assert_allclose(summary["l1_step"], log["l1_step"], rtol=1e-6, atol=0.0)
        np.testing.assert_allclose(summary["last_irls_step"], log["irls_step"][-1], rtol=1e-6, atol=0.0)
    assert summary["num_pcg_stalled_solves"] == 0
    assert np.abs(rot - rot_ref).max() <= rot_tol


@pytest.mark.parametrize("name", ["60_400", "100_800", "300_3000_fixed7", "2000_20000"])
def test_parity_with_the_direct_restatement(name):
    c, rot_ref, log = cases.solved(name)
    rot, summary = device_solve(c)
    assert_same_run(summary, log, rot, rot_ref, 1e-6)
    assert summary["num_edges_used"] == c["edge_i"].shape[0]


def test_theia_four_views_six_pairs_without_noise():
    c = ref.theia_case(4, 6, 0.0, seed=1)
    rot, summary = solver.estimate_rotations_robust_l1l2(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["init_aa"], 0)
    err = ref.relative_to_fixed_error_deg(rot, c["gt_aa"], 0)
    print("largest error %.3e degrees" % err.max())
    assert err.max() < 1e-8


@pytest.mark.parametrize("name", ["hub301_hub_fixed", "hub301_leaf_fixed", "hub70"])
def test_long_rows(name):
    c, rot_ref, log = cases.solved(name)
    assert np.bincount(np.concatenate([c["edge_i"], c["edge_j"]]).astype(np.int64)).max() == c["n_cams"] - 1   # the hub's row
    rot, summary = device_solve(c)
    assert_same_run(summary, log, rot, rot_ref, 1e-6)


def test_edges_as_listed():
    c, rot_ref, log = cases.solved("listed_200_1500")
    assert (c["edge_i"] > c["edge_j"]).sum() > 500 and c["edge_i"].shape[0] == 1650
    rot, summary = device_solve(c)
    assert_same_run(summary, log, rot, rot_ref, 1e-6)


def test_nothing_to_do():
    """Noise-free measurements, started at the ground truth.  With every camera at the identity the residuals are exactly zero, so the
    right-hand sides are: no PCG iteration, and the rotations come back as they went in."""
    g = cases.parity_case("100_800")
    n, E = g["n_cams"], g["edge_i"].shape[0]
    start = np.zeros((n, 3))
    rot, summary = solver.estimate_rotations_robust_l1l2(n, g["edge_i"], g["edge_j"], np.zeros((E, 3)), start, 0)
    assert summary["num_admm_iterations"] == [1] and summary["num_irls_iterations"] == 1
    assert summary["num_cg_iterations"] == 0 and summary["nonfinite"] == 0 and summary["num_pcg_stalled_solves"] == 0
    assert summary["l1_step"] == [0.0] and summary["last_irls_step"] == 0.0
    assert np.all(np.isfinite(rot)) and np.abs(rot - start).max() <= 1e-15


def test_nothing_to_do_at_generic_rotations():
    """The same at generic rotations, where b is rounding error (1e-16) and not zero: the linear solves run on it, both stages stop at
    once, and the rotations move by rounding error.  1e-14: a few ulp of an angle-axis vector of up to pi, twice (in and out)."""
    c = ref.theia_case(50, 300, 0.0, seed=5)
    rot, summary = solver.estimate_rotations_robust_l1l2(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["gt_aa"], 0)
    assert summary["num_admm_iterations"] == [1] and summary["num_irls_iterations"] == 1 and summary["nonfinite"] == 0
    assert np.all(np.isfinite(rot)) and np.abs(rot - c["gt_aa"]).max() <= 1e-14


def test_same_bytes():
    c = cases.parity_case("300_3000_fixed7")
    rot_a, sum_a = device_solve(c)
    rot_b, sum_b = device_solve(c)
    assert rot_a.tobytes() == rot_b.tobytes()
    for s in (sum_a, sum_b):
        del s["t_total_ms"], s["kernel_ms"]
    assert sum_a == sum_b


def test_residual_aid():
    c = cases.residual_case()
    hp = cases.mp_residuals(c)
    out = solver.robust_l1l2_residuals(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["rot_aa"])
    angles = np.linalg.norm(hp, axis=1)
    assert angles[4] < 2e-9 and angles[6] > np.radians(179.8)   # the cases the issue names are in the list
    dev = np.abs(out["b"] - hp)
    print("largest deviation from the 50-digit residuals %.3e (fp64 restatement %.3e)" % (dev.max(), SPREAD["residual"]))
    assert dev.max() <= 4.0 * SPREAD["residual"]
    sq = np.sum(hp * hp, axis=1)
    sigma = ref.DEFAULTS["irls_loss_parameter_sigma"]
    # |b|^2 of a b that is d away from the exact one is off by up to 2 |b| d + d^2 (plus its own rounding)
    d = 4.0 * SPREAD["residual"] * np.sqrt(3.0)
    assert np.all(np.abs(out["sq"] - sq) <= 2.0 * angles * d + d * d + 1e-15 * sq)
    np.testing.assert_allclose(out["weight"], sigma / (sq + sigma * sigma) ** 2, rtol=1e-12)


@pytest.mark.parametrize("form", ["laplacian_weighted", "laplacian_unit"])
def test_laplacian_aid(form):
    lc = cases.laplacian_case()
    w = lc["weights"] if form == "laplacian_weighted" else None
    dense, _, _ = ref.laplacian_solve(lc["n_cams"], lc["edge_i"], lc["edge_j"], lc["rhs"], w, lc["fixed_cam"], linear="dense")
    x, info = solver.robust_l1l2_laplacian_solve(lc["n_cams"], lc["edge_i"], lc["edge_j"], lc["rhs"], w, lc["fixed_cam"], cg_check_interval=1)
    tol = ref.DEFAULTS["cg_relative_tolerance"]
    print("%s: |x - dense| %.3e (restatement %.3e), %d iterations (restatement %d), residual %.3e"
          % (form, np.abs(x - dense).max(), SPREAD[form]["deviation"], info["cg_iterations"], SPREAD[form]["cg_iterations"], info["cg_rel"]))
    assert not info["stalled"] and info["cg_rel"] <= tol
    assert abs(info["cg_iterations"] - SPREAD[form]["cg_iterations"]) <= 2
    assert np.abs(x - dense).max() <= 4.0 * SPREAD[form]["deviation"]
    assert np.all(x[lc["fixed_cam"]] == 0.0)


def test_madrid_from_the_device_spanning_tree():
    n, ei, ej, rel = cases.madrid_graph()
    tree = solver.orientations_from_maximum_spanning_tree(n, ei, ej, rel, weight=None)
    assert tree["n_tree_cams"] == n
    c = cases.madrid_case(init_aa=tree["rot_aa"])
    assert c["fixed_cam"] == tree["root"]
    rot_ref, log = ref.solve(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["init_aa"], c["fixed_cam"], linear="direct")
    print("restatement's margin from the device's start %.3e" % log["margin"])
    rot, summary = device_solve(c)
    assert_same_run(summary, log, rot, rot_ref, 4.0 * SPREAD["madrid"]["deviation"], steps=False)
