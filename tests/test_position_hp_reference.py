"""CPU checks of the high-precision position reference (tests/position_hp_reference.py) against the float64 restatement
(tests/position_reference.py) and the closed forms it must not rely on."""
import mpmath
import numpy as np
import pytest

from globalsfmpy_amd import synth
from globalsfmpy_amd import loss_functions as LF

import hp_reference as H
import position_hp_reference as PH
from position_reference import PositionReference


def _graph(n=12, e=40, seed=2):
    g = synth.make_position_graph(n, e, seed=seed, outlier_frac=0.3, noise=0.01)
    pos = g["gt_pos"] + np.random.default_rng(seed).normal(scale=0.05, size=g["gt_pos"].shape)
    return g, pos


def test_tier1_agrees_with_the_float64_reference_at_generic_points():
    g, pos = _graph()
    ref = PositionReference(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], None)
    r64, u, n, unit = ref.residuals(pos)
    assert unit.all()
    t1 = PH.edge_set(g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], pos)
    np.testing.assert_allclose(t1["d"].astype(float), ref.d, rtol=0, atol=1e-13)
    np.testing.assert_allclose(t1["r"].astype(float), r64, rtol=0, atol=1e-13)
    _, _, A, _, _ = ref.linearize(pos)   # the trivial loss: A = dr/dc_j = (I - u u^T) / n
    scale = 1.0 / n[:, None, None]
    assert np.all(np.abs(t1["Jj"].astype(float) - A) <= 1e-13 * scale)
    assert np.all(t1["Ji"] == -t1["Jj"])


def test_central_differences_give_the_projector_over_n():
    rng = np.random.default_rng(5)
    with mpmath.workdps(PH.MP_DPS):
        for n_target in (1e-11, 1e-3, 1.0, 1e4):
            ci = rng.standard_normal(3)
            w = rng.standard_normal(3)
            cj = ci + n_target * w / np.linalg.norm(w)
            d = [mpmath.mpf(0)] * 3
            r, J, n, unit = PH.edge_linearise(ci, cj, d)
            assert unit
            wm = [mpmath.mpf(float(cj[k])) - mpmath.mpf(float(ci[k])) for k in range(3)]
            um = [x / n for x in wm]
            for a in range(3):
                for b in range(3):
                    exact = ((1 if a == b else 0) - um[a] * um[b]) / n
                    assert abs(J[a][b] - exact) <= mpmath.mpf("1e-20") / n, (n_target, a, b)


@pytest.mark.parametrize("gap", [0.0, 1e-13, 1e-12 * (1 - 1e-6)])
def test_guard_branch_is_the_identity(gap):
    ci = np.array([1e-6, -2e-6, 3e-6])
    cj = ci + np.array([gap, 0.0, 0.0])
    with mpmath.workdps(PH.MP_DPS):
        d = PH.direction([0.1, 0.2, -0.3], [0.0, 1.0, 0.0])
        r, J, n, unit = PH.edge_linearise(ci, cj, d)
        assert not unit and n == 1
        for a in range(3):
            assert r[a] == (mpmath.mpf(float(cj[a])) - mpmath.mpf(float(ci[a]))) - d[a]
            for b in range(3):
                assert abs(J[a][b] - (1 if a == b else 0)) <= mpmath.mpf("1e-17")


def test_guard_is_decided_on_the_exact_norm():
    ci = np.array([1e-6, 0.0, 0.0])
    with mpmath.workdps(PH.MP_DPS):
        for f, unit_expected in ((1 + 1e-6, True), (1 - 1e-6, False)):
            cj = ci + np.array([1e-12 * f, 0.0, 0.0])
            n_exact = abs(mpmath.mpf(float(cj[0])) - mpmath.mpf(float(ci[0])))
            assert abs(n_exact / mpmath.mpf("1e-12") - 1) >= mpmath.mpf("1e-9")
            assert PH.edge_linearise(ci, cj, [mpmath.mpf(0)] * 3)[3] == unit_expected


@pytest.mark.parametrize("loss,kind,params", [(LF.TukeyLoss(0.5), "tukey", (0.5,)), (LF.GemanMcClureLoss(0.3, 0.5), "geman_mcclure", (0.3, 0.5)),
                                              (LF.ScaledLoss(LF.HuberLoss(0.5), 2.5), "scaled", (("huber", (0.5,)), 2.5)),
                                              (LF.TolerantLoss(0.05, 0.1), "tolerant", (0.05, 0.1))])
def test_long_double_losses_match_loss_functions(loss, kind, params):
    s = np.concatenate([[0.0, 1e-12, 0.2, 0.25 * (1 - 1e-9), 0.25 * (1 + 1e-9), 1.0, 4.0], np.random.default_rng(1).uniform(0, 4, 50)])
    r0, r1, r2, scale = PH.loss_rho(kind, params, s)
    for k, v in enumerate(s):
        out = [0.0, 0.0, 0.0]
        loss.Evaluate(float(v), out)
        # (the float64 formula of rho itself may lose digits to cancellation: it is held to its own evaluation scale)
        assert abs(float(r0[k]) - out[0]) <= 1e-14 * float(scale[k]), (k, v)
        np.testing.assert_allclose([float(r1[k]), float(r2[k])], out[1:], rtol=1e-13, atol=1e-300)
        assert float(scale[k]) >= abs(float(r0[k])) * (1 - 1e-15)


@pytest.mark.parametrize("kind,params,loss", [(None, (), None), ("huber", (0.1,), LF.HuberLoss(0.1)), ("tolerant", (0.05, 0.1), LF.TolerantLoss(0.05, 0.1))])
def test_step_system_matches_the_float64_first_step(kind, params, loss):
    g, pos = _graph(14, 50, seed=9)
    fixed = 3
    ref = PositionReference(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], loss)
    ref.solve(pos, fixed_cam=fixed, max_num_iterations=1, record_steps=1)
    st = ref.steps[0]
    lin = PH.corrected(PH.edge_set(g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], pos), kind, params)
    active = ref.present.copy()
    active[fixed] = False
    sysm = PH.step_system(lin, g["n_cams"], g["edge_i"], g["edge_j"], active, st["radius"])
    y = PH.solve_refined(sysm["K"], sysm["b"])
    idx = st["idx"]
    np.testing.assert_allclose(sysm["b"][idx].astype(float), st["rhs"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(sysm["K"][np.ix_(idx, idx)].astype(float), st["K"].toarray(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(y[idx].astype(float), st["y"], rtol=1e-9, atol=1e-12)
    assert np.all(y[~sysm["act"]] == 0)
    delta, v, mcc, dg, dld = PH.project_step(y, sysm, pos, fixed)
    np.testing.assert_allclose(delta.astype(float), st["delta"], rtol=1e-9, atol=1e-12)
    assert abs(float(delta @ v)) <= 1e-15 * float(np.sqrt(delta @ delta) * np.sqrt(v @ v))
    assert mcc > 0
