"""The numpy / scipy restatement of the robust L1 + IRLS rotation estimator (tests/robust_rotation_reference.py) on its own: Theia's three
test cases, the agreement of its linear solvers, the decision margin of every input the GPU tests use, and the recorded spreads of
tests/golden/robust_rotation_spread.json."""
import json
import os
import sys

import numpy as np
import pytest

import robust_rotation_cases as cases
import robust_rotation_reference as ref

sys.path.insert(0, cases.GOLDEN)
import make_robust_rotation_spread as maker   # noqa: E402


# views, pairs, noise (degrees), bound (degrees): robust_rotation_estimator_test.cc
@pytest.mark.parametrize("n_views,n_pairs,noise,bound", [(4, 6, 0.0, 1e-8), (4, 6, 1.0, 1.0), (100, 800, 2.0, 5.0)])
def test_theia_cases(n_views, n_pairs, noise, bound):
    for seed in (1, 2, 3):
        c = ref.theia_case(n_views, n_pairs, noise, seed)
        rot, log = ref.solve(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["init_aa"], 0)
        err = ref.relative_to_fixed_error_deg(rot, c["gt_aa"], 0)   # relative to the fixed camera, no alignment
        print("%d / %d, %g degrees of noise, seed %d: largest error %.3e degrees, admm %s, irls %d" % (n_views, n_pairs, noise, seed, err.max(),
                                                                                                      log["admm_iterations"], log["irls_iterations"]))
        assert err.max() < bound
        assert err[0] == 0.0


def test_the_linear_solvers_agree():
    c, rot, log = cases.solved("300_3000_fixed7")
    for linear in ("dense", "pcg"):
        rot2, log2 = ref.solve(c["n_cams"], c["edge_i"], c["edge_j"], c["rel_aa"], c["init_aa"], c["fixed_cam"], linear=linear)
        assert log2["admm_iterations"] == log["admm_iterations"] and log2["irls_iterations"] == log["irls_iterations"]
        assert np.abs(rot2 - rot).max() < 1e-10
    assert np.all(rot[c["fixed_cam"]] == c["init_aa"][c["fixed_cam"]])


def test_an_edge_list_in_another_order_and_a_camera_without_edges():
    c, rot, log = cases.solved("60_400")
    perm = np.random.default_rng(0).permutation(c["edge_i"].shape[0])
    init = np.vstack([c["init_aa"], [[0.3, -0.2, 0.1]]])   # camera 60 appears in no edge
    rot2, log2 = ref.solve(61, c["edge_i"][perm], c["edge_j"][perm], c["rel_aa"][perm], init, c["fixed_cam"])
    assert log2["admm_iterations"] == log["admm_iterations"] and np.abs(rot2[:60] - rot).max() < 1e-10
    assert np.all(rot2[60] == init[60])


@pytest.mark.parametrize("name", sorted(cases.SOLVE_CASES))
def test_decision_margin_of_the_gpu_inputs(name):
    """A condition on the inputs: no compared quantity of the direct restatement comes closer than 1e-4 (relative) to its threshold, so
    an implementation that agrees with it to 1e-6 takes the same decisions."""
    c, rot, log = cases.solved(name)
    print("%s: margin %.3e, admm %s, irls %d" % (name, log["margin"], log["admm_iterations"], log["irls_iterations"]))
    assert log["margin"] >= 1e-4
    assert np.all(np.isfinite(rot))


def test_the_host_spanning_tree_reaches_every_madrid_camera():
    n, ei, ej, rel = cases.madrid_graph()
    start, root, seen = cases.tree_start(n, ei, ej, rel)
    assert seen.all() and root == 0 and np.all(start[root] == 0.0)


def test_recorded_spreads_match_the_restatement():
    """tests/golden/robust_rotation_spread.json against what make_robust_rotation_spread.py computes now: the counts exactly; the
    deviations, which are rounding error and change with the order of a library's sums, to a factor of 2 either way (the GPU tests allow
    the device 4 x the recorded figure)."""
    with open(maker.OUT) as f:
        recorded = json.load(f)
    now = maker.compute(with_table=False)
    assert recorded["madrid"]["cg_relative_tolerance"] == ref.DEFAULTS["cg_relative_tolerance"]
    for key in ("admm_iterations", "irls_iterations", "direct_admm_iterations", "direct_irls_iterations", "cg_iterations"):
        assert recorded["madrid"][key] == now["madrid"][key], key
    assert recorded["madrid"]["admm_iterations"] == recorded["madrid"]["direct_admm_iterations"]
    assert recorded["madrid"]["irls_iterations"] == recorded["madrid"]["direct_irls_iterations"]
    pairs = [(recorded["residual"], now["residual"]), (recorded["madrid"]["deviation"], now["madrid"]["deviation"])]
    for form in ("laplacian_weighted", "laplacian_unit"):
        assert recorded[form]["cg_iterations"] == now[form]["cg_iterations"]
        pairs.append((recorded[form]["deviation"], now[form]["deviation"]))
    for rec, cur in pairs:
        assert rec > 0.0 and 0.5 * rec <= cur <= 2.0 * rec, (rec, cur)
    assert [row["cg_relative_tolerance"] for row in recorded["madrid_by_tolerance"]] == [1e-10, 1e-12, 1e-14, 1e-15]
