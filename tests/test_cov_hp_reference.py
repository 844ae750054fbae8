"""The high-precision reference of the per-edge covariance (tests/cov_hp_reference.py) against the CPU oracle, on the CPU: tier 1
(the signed Sampson residual, its Jacobian in the reference's five parameters, the chart's Plus and Jacobian on both pole branches)
within double-precision bounds, and tier 2 (the covariance at a fixed pose, one LM iteration) at generic, well-conditioned points."""
import numpy as np
import pytest

import cov_hp_reference as CR

U = CR.U


def _edge(seed, n=40, **kw):
    return CR.make_edge(seed, n, **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tier1_residual_and_jacobian_match_the_oracle(oracle, seed):
    m, K, r, t = _edge(seed, 12, t=np.array([0.4, -0.7, 0.6]) * 1.7)
    s, J, sc = CR.edge_tier1(m, K, r, t)
    Jh = oracle.homogeneous_jacobian(t)
    for i in range(len(m)):
        ro, jac = oracle.sampson_residual(m[i], K, r, t, want_jacobian=True)
        sg = 1.0 if s[i] >= 0 else -1.0
        # the oracle forms num in pixel coordinates (its terms are f times larger before they cancel): 1e3 u of the scale
        assert abs(ro - abs(float(s[i]))) <= 1e3 * U * float(sc[i]), (i, ro, float(s[i]))
        jo = np.r_[jac[:3], jac[3:] @ Jh]
        assert np.all(np.abs(jo - sg * J[i].astype(float)) <= 1e3 * U * float(sc[i])), (i, jo, J[i])


@pytest.mark.parametrize("x", [[0.3, -0.2, 0.9], [0, 0, 1.0], [0, 0, -1.0], [1e-8, 0, 1.0], [1e-8, 0, -1.0], [2e-8, 0, 1.0],
                               [2e-8, 0, -1.0], [0, 0, 2.5], [1e-8, 0, -2.5]])
def test_chart_plus_and_jacobian_match_the_oracle_on_both_pole_branches(oracle, x):
    assert CR.branch_exact_agrees(x)
    nx = float(np.linalg.norm(x))
    for d in ([0.1, -0.2], [1e-3, 2e-3], [-0.5, 0.25]):
        assert np.all(np.abs(CR.hom_plus_f(x, d) - oracle.homogeneous_plus(x, d)) <= 16 * U * nx), (x, d)
    assert np.all(np.abs(CR.hom_jacobian_fd(x) - oracle.homogeneous_jacobian(x)) <= 16 * U * nx), x


def test_pole_branch_is_decided_on_the_double_sigma():
    # sigma = fl(1e-16) <= DBL_EPSILON: the branch (Plus tends to |x| e_z, Jacobian 0.5 |x| [I; 0]); 2e-8: off the branch
    J = CR.hom_jacobian_fd([1e-8, 0, 1.0])
    assert np.array_equal(J, np.array([[0.5, 0], [0, 0.5], [0, 0]]))
    assert CR.hom_plus_f([1e-8, 0, 1.0], [1e-300, 0])[0] < 1e-20
    assert abs(CR.hom_plus_f([2e-8, 0, 1.0], [1e-300, 0])[0] - 2e-8) < 1e-20


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_tier2_covariance_at_a_fixed_pose_matches_the_oracle(oracle, seed):
    m, K, r, t = _edge(seed, 80)
    ed = CR.edge_data(m, K, r, t)
    assert ed["kappa"] < 1e4 and ed["pivot_ratio"] > 1e-6
    b = CR.batch([(m, K, r, t)])
    o = oracle.estimate_rotation_covariances(b["match_ptr"], b["matches"], b["intrinsics"], b["rot"], b["trans"], max_iterations=0)
    assert o["status"][0] == 0 and o["iterations"][0] == 0
    # the oracle's own double evaluation, in pixel coordinates, with a 1e3 u bound per j component of the scale
    bound = CR.cov_bound(ed, 1e3, 1e3, 64)
    assert CR.ratio(o["cov"][0], ed["C"], bound) <= 1.0
    assert CR.allowed_relative(bound, np.abs(ed["C"])) <= 1e-9


@pytest.mark.parametrize("seed,off", [(7, 0.0), (8, 0.3)])
def test_tier2_one_lm_iteration_matches_the_oracle(oracle, seed, off):
    m, K, r, t = _edge(seed, 60, t=np.array([0.62, 0.3, -0.72]) * 2.0)
    r = r + CR.aa(off, [0.2, 1.0, -0.4]) if off else r
    ed = CR.edge_data(m, K, r, t)
    st = CR.lm_step(m, K, r, t, ed)
    assert st["accept"] and st["rel_dec_margin"] > 2 and st["func_margin"] > 10 and st["param_margin"] > 10
    b = CR.batch([(m, K, r, t)])
    o = oracle.estimate_rotation_covariances(b["match_ptr"], b["matches"], b["intrinsics"], b["rot"], b["trans"], max_iterations=1)
    assert o["iterations"][0] == 1
    step = np.abs(st["delta"].astype(float))
    assert np.all(np.abs(o["rotation"][0] - st["crot"].astype(float)) <= 1e-9 * step[:3].max() + 4 * U * np.abs(r).max())
    assert np.all(np.abs(o["translation"][0] - st["ct"].astype(float)) <= 1e-9 * np.linalg.norm(t) * step[3:].max() + 64 * U * np.linalg.norm(t))
    # the model's cost change against the realised one: both from the reference (a correct step has rel_dec near 1)
    assert abs(float(st["rel_dec"]) - 1.0) < 0.1
