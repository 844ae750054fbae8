"""The high-precision reference (tests/hp_reference.py) checked against the CPU oracle and against itself -- no GPU needed.

At generic points the oracle's double-precision Ceres route and the 40-digit finite differences must agree to 1e-12 relative:
that settles every convention (parameterisation, residual order, whitening, canonicalisation).  The long-double losses and
Corrector are checked against the same formulas in mpmath."""
import mpmath
import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth

import hp_reference as H


@pytest.fixture(scope="module")
def graph():
    return synth.make_graph(n_cams=16, n_edges=30, seed=3, outlier_frac=0.2, full_so3=True)


@pytest.mark.parametrize("et", list(range(9)))
def test_tier1_matches_oracle_at_generic_points(oracle, graph, et):
    g = graph
    ref = H.edge_set(et, g["edge_i"], g["edge_j"], g["rel_aa"], g["init_aa"], g["cov6"], g["inlier_weight"])
    o = oracle.OracleProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"], inlier_weight=g["inlier_weight"])
    rs = o.residuals(g["init_aa"], want_residuals=True)["residuals"]
    for e in range(len(g["edge_i"])):
        r, Ji, Jj = o.edge_jacobians(e, g["init_aa"])
        sr = max(1.0, float(np.abs(ref["r"][e]).max()))
        assert np.abs(r - ref["r"][e]).max() <= 1e-12 * sr, (e, r, ref["r"][e])
        assert np.abs(rs[e] - ref["r"][e]).max() <= 1e-12 * sr
        for J, Jr in ((Ji, ref["Ji"][e]), (Jj, ref["Jj"][e])):
            assert np.abs(J - Jr).max() <= 1e-12 * max(1.0, float(np.abs(Jr).max())), (e, J, Jr)
        if et in H.AA_TYPES:
            W = oracle.whitening(et, g["cov6"][e], g["inlier_weight"][e])
            assert np.abs(W - ref["W"][e]).max() <= 1e-12 * max(1.0, np.abs(ref["W"][e]).max())


@pytest.mark.parametrize("et", [_abi.ANGLE_AXIS, _abi.QUATERNION_NORM])
def test_tier1_linearize_matches_oracle(oracle, graph, et):
    g = graph
    ref = H.edge_set(et, g["edge_i"], g["edge_j"], g["rel_aa"], g["init_aa"], g["cov6"], g["inlier_weight"])
    o = oracle.OracleProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"], inlier_weight=g["inlier_weight"])
    from globalsfmpy_amd import loss_functions as LF
    o.set_loss(LF.TolerantLoss(0.05, 0.01))
    A = H.assemble(H.corrected(ref, "tolerant", (0.05, 0.01)), g["n_cams"], g["edge_i"], g["edge_j"])
    b = o.linearize(g["init_aa"])
    assert np.abs(b["gradient"] - A["g"]).max() <= 1e-12 * float(np.abs(A["g_mag"]).max())
    assert np.abs(b["diag_blocks"] - A["D"]).max() <= 1e-12 * float(np.abs(A["D_mag"]).max())
    assert abs(b["cost"] - float(A["cost"])) <= 1e-12 * abs(float(A["cost"]))


def _mp_loss(kind, p, s):
    s = mpmath.mpf(s)
    if kind == "huber":
        a = mpmath.mpf(p[0])
        if s > a * a:
            return 2 * a * mpmath.sqrt(s) - a * a, a / mpmath.sqrt(s), -a / mpmath.sqrt(s) / (2 * s)
        return s, mpmath.mpf(1), mpmath.mpf(0)
    if kind == "softl1":
        b = mpmath.mpf(p[0]) ** 2
        t = 1 + s / b
        return 2 * b * (mpmath.sqrt(t) - 1), 1 / mpmath.sqrt(t), -1 / (2 * b * t ** mpmath.mpf(1.5))
    if kind == "cauchy":
        b = mpmath.mpf(p[0]) ** 2
        return b * mpmath.log(1 + s / b), 1 / (1 + s / b), -1 / (b * (1 + s / b) ** 2)
    a, b = mpmath.mpf(p[0]), mpmath.mpf(p[1])
    x = (s - a) / b
    c = b * mpmath.log(1 + mpmath.exp(-a / b))
    if x > mpmath.mpf(36.7):   # the reference's linear branch
        return s - a - c, mpmath.mpf(1), mpmath.mpf(0)
    return b * mpmath.log(1 + mpmath.exp(x)) - b * mpmath.log(1 + mpmath.exp(-a / b)), 1 / (1 + mpmath.exp(-x)), 1 / (2 * b * (1 + mpmath.cosh(x)))


@pytest.mark.parametrize("kind,params", [("huber", (0.5,)), ("softl1", (0.3,)), ("cauchy", (0.2,)), ("tolerant", (0.05, 0.01))])
def test_tier2_losses_match_mpmath(kind, params):
    """rho, rho', rho'' in long double against mpmath, each to ~1e3 long-double units of its own evaluation scale."""
    s = np.array([0.0, 1e-12, 1e-6, 0.01, 0.0499, 0.0501, 0.2499, 0.2501, 0.3, 1.0, 7.0])
    rho = H.loss_rho(kind, params, s)
    eps = float(np.finfo(H.LD).eps)
    with mpmath.workdps(40):
        for k, sk in enumerate(s):
            ref = _mp_loss(kind, params, sk)
            for d in range(3):
                err = abs(mpmath.mpf(str(rho[d][k])) - ref[d])
                scale = (rho[3][k] if d == 0 else 0) + abs(ref[d]) + (abs(ref[d + 1]) * sk if d < 2 else 0)
                assert err <= 1e3 * eps * float(scale) + 1e-300, (kind, sk, d, float(err))
