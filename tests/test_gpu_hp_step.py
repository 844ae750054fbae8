"""-m gpu: one rotation LM step's linear solve -- the PCG recurrences with their fused mat-vecs, the two-level correction, the damped blocks,
the chunk loop with hipGraph replay and parity, the mixed dense / PCG component step, the exact step and k_cam_step's sums -- against the
high-precision normal system of the same step (tests/hp_reference.py).  Every case is one RotationProblem.step_check call
(gsfm_rot_step_check: the solve's own phases, stopped before the trust-region decision).

A full solve cannot see a wrong step: the fixed point of LM depends on the gradient alone.  Here the device's step delta (in the
reference's parameters) is put into the reference's system K* = H* + diag(lam*), b* = -g*:

  true relative residual  sqrt(r.M^-1 r / b.M^-1 b), r = b* - K* delta   <=   cg_rel (what the device reports) + floor
  floor = || C0 u (|K*||delta| + |b*|) + c_row(deg, 16) u (|K*||delta| + g_mag) ||_{M^-1} / ||b*||_{M^-1}      (hp_reference.step_residual)

with C0 = 64 and c_row as in test_gpu_hp_linearization.py.  The floor is what a double-precision evaluation of the residual at delta can be
off by; it also covers the u-level rounding of forming delta = Tinv eta on the host.  Before the device result is looked at, every case
asserts that the floor at the exact solution is at most tol / 2 = 5e-13 (measured on the CPU: 1.3e-13 to 4.1e-13,
tests/test_hp_step_reference.py), so a step that is off by 1e-12 relative fails.

Further, per case: the path and the switches are the ones forced; the tolerance the kernels tested against is 1e-12 (the 2e-14 rad
absolute floor does not bind on steps of 0.1 to 1 rad); delta is exactly zero on cameras without an edge; x_trial = Plus(x, delta) to 4 u on
the magnitudes of the component's terms (additive: |x| + |delta| + 2 |eta|_2, the last for the two roundings of Tinv eta -- |Tinv|_2 < 2 for
states below 1 rad, asserted; quaternion: the four products of the quaternion product, delta = eta / 2 being exact); the model cost change
from the device's sums against the reference's at the device's delta; S3, S4 against |x - x_trial|^2, |x_trial|^2 to (C0 + N) u.

Every test prints its worst ratio observed / bound (pytest -s); DESIGN.md section 2 records them.
"""
import numpy as np
import pytest

from globalsfmpy_amd import _abi
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem

import hp_reference as H
import position_hp_reference as PH

pytestmark = pytest.mark.gpu

U, LD = H.U, H.LD
C0 = 64.0
TOL = 1e-12
LOSS_OBJ = {"none": None, "huber": LF.HuberLoss(0.5), "tolerant": LF.TolerantLoss(0.05, 0.01)}
PCG = {"dense_cholesky_max_cams": 0}   # every PCG case: no exact step, no rescue by the factorisation
TEXTBOOK, SINGLE = _abi.STEP_PCG_TEXTBOOK, _abi.STEP_PCG_SINGLE_REDUCTION
RECURRENCES = [(0, TEXTBOOK), (1, SINGLE)]


def _device(name, et, lname, callback=False):
    g = H.step_graph(name)
    dev = RotationProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"], inlier_weight=g["inlier_weight"])
    if callback:
        dev.set_loss_callback(LOSS_OBJ[lname].Evaluate)
    else:
        dev.set_loss(LOSS_OBJ[lname])
    return dev


def _floor_condition(case):
    """the reference's own floor at the exact solution, asserted before any device result is looked at"""
    name, et, lname, radius = case
    g, lin, A, sysm = H.step_reference(*case)
    xs = H.step_solution(*case)
    _, floor, _ = H.step_residual(lin, A, sysm, g["n_cams"], g["edge_i"], g["edge_j"], xs)
    assert floor <= H.STEP_FLOOR_MAX, (case, floor)
    return floor


def _plus_ratio(res):
    """x_trial against Plus(x, delta) in long double, worst error / (4 u magnitude)"""
    x, xt, d = res["x"].astype(LD), res["x_trial"].astype(LD), res["delta"].astype(LD)
    if x.shape[1] == 3:
        assert np.all(np.sqrt((res["x"] ** 2).sum(axis=1)) < 1.0)   # |Tinv|_2 <= 1 + theta / 2 + theta^2 / 10 < 2
        en = np.sqrt((res["eta"].astype(LD) ** 2).sum(axis=1))[:, None]
        return H.ratio(xt, x + d, 4 * U * (np.abs(x) + np.abs(d) + 2 * en))
    nd = np.sqrt((d * d).sum(axis=1))
    safe = np.where(nd > 0, nd, 1)
    k = np.where(nd > 0, np.sin(safe) / safe, 1)
    ax, ay, az, aw = k * d[:, 0], k * d[:, 1], k * d[:, 2], np.where(nd > 0, np.cos(safe), 1)
    bx, by, bz, bw = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    terms = [(aw * bx, ax * bw, ay * bz, -az * by), (aw * by, ay * bw, az * bx, -ax * bz), (aw * bz, az * bw, ax * by, -ay * bx),
             (aw * bw, -ax * bx, -ay * by, -az * bz)]
    ref = np.stack([sum(t) for t in terms], axis=1)
    mag = np.stack([sum(np.abs(v) for v in t) for t in terms], axis=1)
    return H.ratio(xt, ref, 4 * U * mag)


def _check_step(res, case, worst, capped=False, tol=TOL):
    """The assertions every PCG-solved (or exact) step gets; fills `worst` with observed / bound."""
    name, et, lname, radius = case
    g, lin, A, sysm = H.step_reference(*case)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    delta = res["delta"]
    assert np.all(np.isfinite(delta)) and np.all(np.isfinite(res["x_trial"]))
    rel, floor, r = H.step_residual(lin, A, sysm, n, ei, ej, delta)
    pcg = res["path"] != _abi.STEP_DENSE   # (the component step of the tests has a PCG-solved component)
    if pcg:
        assert res["cg_tolerance"] == tol, res["cg_tolerance"]
        if capped:
            assert res["cg_rel"] > tol
            worst["recursive_vs_true"] = abs(rel - res["cg_rel"]) / floor
        else:
            assert res["cg_rel"] <= tol, res["cg_rel"]
    worst["residual"] = rel / (res["cg_rel"] + floor)
    # the damping diagonal the device built, in the reference's parameters: c_row roundings on D*'s diagonal, then ~10 of its own
    Dm = np.stack([A["D_mag"][:, c, c] for c in range(3)], axis=1)
    dd = np.stack([A["D"][:, c, c] for c in range(3)], axis=1)
    rel_dd = H.c_row(A["deg"], 16.0)[:, None] * U * np.where(dd > 0, Dm / np.where(dd > 0, dd, 1), 0)
    worst["lam"] = H.ratio(res["lam"], sysm["lam"], sysm["lam"] * (rel_dd + C0 * U))
    worst["plus"] = _plus_ratio(res)
    # model cost change from the device's sums against the reference's at the device's delta (positions test, _delta_checks, with the
    # rotation quantities): the host-formed delta is within dd of the device's own; the sums' roundings; and the recursive residual the
    # device's sum S1 uses against the true one -- at most ||r_true|| + ||r_cg|| <= (2 cg_rel + floor) ||b|| in the M^-1 norm
    mcc, mag = H.model_cost_change(lin, A, n, ei, ej, delta)
    d64 = delta.astype(LD)
    eta_n = float(np.sqrt((res["eta"].astype(LD) ** 2).sum()))
    ddel = 6 * U * 2 * eta_n
    gn = float(np.sqrt((A["g"] ** 2).sum()))
    dn = float(np.sqrt((d64 ** 2).sum()))
    K = _system_matrix(case)
    normH = float(np.abs(K).sum(axis=1).max())   # (>= |K|_2 >= |H|_2 for the symmetric K)
    lam_mag = float((sysm["lam"] * d64 * d64).sum())
    dM = float(np.sqrt(np.einsum("ka,kab,kb->", d64, sysm["M"], d64)))
    bn = float(H.mnorm(sysm, sysm["b"]))
    mb = ddel * (gn + normH * (dn + ddel)) + (C0 + 3 * n) * U * (float(mag) + lam_mag) + 0.5 * dM * (2 * res["cg_rel"] + floor) * bn
    worst["model"] = abs(float(LD(res["model_cost_change"]) - mcc)) / mb
    assert mcc > 0
    # S3, S4
    x, xt = res["x"].astype(LD), res["x_trial"].astype(LD)
    act = (A["deg"] > 0)[:, None]
    s3, s4 = ((x - xt) ** 2).sum(), (np.where(act, xt, 0) ** 2).sum()
    worst["S3"] = abs(float(LD(res["step_sums"][3]) - s3)) / float((C0 + n) * U * s3)
    worst["S4"] = abs(float(LD(res["step_sums"][4]) - s4)) / float((C0 + n) * U * s4)
    assert np.all(delta[A["deg"] == 0] == 0.0)
    return rel, floor


_K = {}


def _system_matrix(case):
    if case not in _K:
        g, lin, A, sysm = H.step_reference(*case)
        _K[case] = H.system_matrix(lin, sysm, g["n_cams"], g["edge_i"], g["edge_j"])
    return _K[case]


def _report(tag, res, worst, extra=""):
    print("step %-46s path %d cg %4d rel %.2e | %s %s" % (tag, res["path"], res["cg_iterations"], res["cg_rel"],
                                                         " ".join("%s %.3f" % kv for kv in sorted(worst.items())), extra))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _run(dev, case, tag, expect_path, capped=False, **opts):
    rot = H.step_graph(case[0])["rot"]
    o = dict(PCG)
    o.update(opts)
    res = dev.step_check(rot, radius=case[3], **o)
    assert res["path"] == expect_path, (tag, res["path"])
    worst = {}
    _check_step(res, case, worst, capped=capped)
    _report(tag, res, worst)
    return res


MAIN = ("main", _abi.ANGLE_AXIS, "huber", 1e4)


# ---- recurrences, graph replay, radius, check interval ---------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e4, 1e12])
@pytest.mark.parametrize("sr,path", RECURRENCES)
def test_recurrences_with_and_without_graph_replay(radius, sr, path):
    case = ("main", _abi.ANGLE_AXIS, "huber", radius)
    _floor_condition(case)
    dev = _device(*case[:3])
    a = _run(dev, case, "graph sr=%d r=%.0e" % (sr, radius), path, pcg_single_reduction=sr, pcg_hip_graph=1)
    b = _run(dev, case, "plain sr=%d r=%.0e" % (sr, radius), path, pcg_single_reduction=sr, pcg_hip_graph=0)
    dev.close()
    assert a["graph_launches"] > 0 and b["graph_launches"] == 0
    assert a["lin_is_lap"] == 1 and a["column_sorted"] == 0 and a["coarse_n"] == 0
    assert a["eta"].tobytes() == b["eta"].tobytes() and a["cg_iterations"] == b["cg_iterations"]


@pytest.mark.parametrize("sr,path", RECURRENCES)
def test_check_interval_does_not_change_the_iterates(sr, path):
    _floor_condition(MAIN)
    dev = _device(*MAIN[:3])
    base = _run(dev, MAIN, "interval 8 sr=%d" % sr, path, pcg_single_reduction=sr)
    for interval, graphs in ((2, True), (5, False)):
        r = _run(dev, MAIN, "interval %d sr=%d" % (interval, sr), path, pcg_single_reduction=sr, cg_check_interval=interval)
        assert (r["graph_launches"] > 0) == graphs, (interval, r["graph_launches"])
        assert r["eta"].tobytes() == base["eta"].tobytes() and r["cg_iterations"] == base["cg_iterations"]
    dev.close()


# ---- forced layouts ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    "general_blocks": ({"GSFM_LAPLACIAN": "0"}, {"lin_is_lap": 0, "column_sorted": 0}),
    "colsort": ({"GSFM_K3_COLSORT": "1"}, {"lin_is_lap": 1, "column_sorted": 1}),
    "colsort_k16": ({"GSFM_K3_COLSORT": "1", "GSFM_K3C_K16": "1"}, {"lin_is_lap": 1, "column_sorted": 1}),
    "row_lanes_1": ({"GSFM_ROW_LANES": "1"}, {"lin_is_lap": 1, "column_sorted": 0}),
    "row_lanes_64": ({"GSFM_ROW_LANES": "64"}, {"lin_is_lap": 1, "column_sorted": 0}),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_forced_layouts(monkeypatch, layout):
    env, flags = LAYOUTS[layout]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _floor_condition(MAIN)
    dev = _device(*MAIN[:3])
    for sr, path in RECURRENCES:
        r = _run(dev, MAIN, "%s sr=%d" % (layout, sr), path, pcg_single_reduction=sr)
        assert {k: r[k] for k in flags} == flags, (layout, r)
        assert r["graph_launches"] > 0
    dev.close()


# ---- two-level correction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_agg", [4, 2])
def test_two_level_correction(monkeypatch, n_agg):
    """4 aggregates of 150 cameras (below a block of the camera kernels: the restriction is its own kernel), 2 of 300 (fused into
    k_cg_update).  The coarse space runs with the textbook recurrence only.  Iteration counts printed beside block-Jacobi's, not asserted."""
    _floor_condition(MAIN)
    plain = _device(*MAIN[:3])
    bj = _run(plain, MAIN, "block-Jacobi textbook", TEXTBOOK, pcg_single_reduction=0)
    plain.close()
    monkeypatch.setenv("GSFM_PCG_COARSE", str(n_agg))
    dev = _device(*MAIN[:3])
    r = _run(dev, MAIN, "coarse %d" % n_agg, TEXTBOOK)
    dev.close()
    assert r["coarse_n"] == n_agg and r["lin_is_lap"] == 1 and r["graph_launches"] > 0
    print("two-level correction, %d aggregates: %d PCG iterations (block-Jacobi %d)" % (n_agg, r["cg_iterations"], bj["cg_iterations"]))


# ---- error types and losses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("et", [_abi.QUATERNION_COSINE, _abi.QUATERNION_NORM, _abi.ANGLE_AXIS_COVARIANCE, _abi.ANGLE_AXIS_COV_INLIERS])
def test_error_types(et):
    case = ("main", et, "huber", 1e4)
    _floor_condition(case)
    dev = _device(*case[:3])
    for sr, path in RECURRENCES:
        r = _run(dev, case, "et %d sr=%d" % (et, sr), path, pcg_single_reduction=sr)
        assert r["x"].shape[1] == (3 if et in H.AA_TYPES else 4)
        if et == _abi.QUATERNION_NORM:
            assert r["lin_is_lap"] == 0
    dev.close()


@pytest.mark.parametrize("lname", ["none", "tolerant"])
def test_losses(lname):
    case = ("main", _abi.ANGLE_AXIS, lname, 1e4)
    _floor_condition(case)
    dev = _device(*case[:3])
    for sr, path in RECURRENCES:
        _run(dev, case, "loss %s sr=%d" % (lname, sr), path, pcg_single_reduction=sr)
    dev.close()


def test_host_callback_loss():
    case = ("main", _abi.ANGLE_AXIS, "tolerant", 1e4)
    _floor_condition(case)
    dev = _device(*case[:3], callback=True)
    _run(dev, case, "callback tolerant", SINGLE)
    dev.close()


# ---- iteration cap: the recursive residual is honest when it is large, too --------------------------------------------------------------
@pytest.mark.parametrize("sr,path", RECURRENCES)
def test_iteration_cap(sr, path):
    _floor_condition(MAIN)
    dev = _device(*MAIN[:3])
    r = _run(dev, MAIN, "cap 6 sr=%d" % sr, path, capped=True, pcg_single_reduction=sr, max_cg_iterations=6)
    dev.close()
    assert r["cg_iterations"] == 6


# ---- components ---------------------------------------------------------------------------------------------------------------------------
def test_component_step():
    """A component of 36 cameras factorised beside one of 300 solved by PCG (dense_cholesky_max_cams = 40), two cameras without an edge."""
    case = ("twocomp", _abi.ANGLE_AXIS, "huber", 1e4)
    _floor_condition(case)
    g, lin, A, sysm = H.step_reference(*case)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    assert sorted(np.bincount(g["comp"])) == [2, 36, 300] and np.all(A["deg"][g["comp"] == 2] == 0)
    dev = _device(*case[:3])
    # component_rest = 0: the reference's single stopping rule.  (With the default, a disconnected problem's PCG has an absolute floor of
    # 1e-11 rad per camera instead of 2e-14 -- include/gsfm_rot.h, component_rest -- which binds here: the kernels then test against 1.15e-12.)
    res = dev.step_check(g["rot"], radius=1e4, dense_cholesky_max_cams=40, component_rest=0)
    dev.close()
    assert res["path"] == _abi.STEP_COMPONENTS and res["dense_info"] == 0 and res["cg_iterations"] > 0
    worst = {}
    _check_step(res, case, worst)   # (the whole system: <= cg_rel + floor)
    assert np.all(res["delta"][g["comp"] == 2] == 0.0) and np.all(res["eta"][g["comp"] == 2] == 0.0)
    big, small = np.flatnonzero(g["comp"] == 0), np.flatnonzero(g["comp"] == 1)
    rb, fb, _ = H.step_residual(lin, A, sysm, n, ei, ej, res["delta"], cams=big)
    rs, fs, _ = H.step_residual(lin, A, sysm, n, ei, ej, res["delta"], cams=small)
    assert fb <= H.STEP_FLOOR_MAX and fs <= H.STEP_FLOOR_MAX
    worst["pcg_component"] = rb / (res["cg_rel"] + fb)
    worst["dense_component"] = rs / fs
    # (K* is block diagonal over the components: each residual above is the component's own solve's, and a step mixed up between the
    # components or scattered to the wrong cameras fails them)
    _report("components 36 + 300 + 2 isolated", res, worst)


# ---- loose, then resumed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,path", RECURRENCES)
def test_loose_then_resumed_equals_uninterrupted(sr, path):
    _floor_condition(MAIN)
    g, lin, A, sysm = H.step_reference(*MAIN)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    dev = _device(*MAIN[:3])
    tight = _run(dev, MAIN, "tight sr=%d" % sr, path, pcg_single_reduction=sr)
    tau = 1e-3
    o = dict(PCG)
    res = dev.step_check(g["rot"], radius=1e4, loose_tau=tau, pcg_single_reduction=sr, **o)
    dev.close()
    assert res["path"] == path
    assert 0 < res["loose_cg_iterations"] < res["cg_iterations"] and res["loose_cg_rel"] > TOL
    assert res["eta"].tobytes() == tight["eta"].tobytes() and res["cg_iterations"] == tight["cg_iterations"]
    assert res["step_sums"].tobytes() == tight["step_sums"].tobytes()
    worst = {}
    _check_step(res, MAIN, worst)
    xs = H.step_solution(*MAIN)
    e = res["delta_loose"].astype(LD) - xs
    Ke, _, _ = H.system_apply(lin, sysm, n, ei, ej, e)
    Kx, _, _ = H.system_apply(lin, sysm, n, ei, ej, xs)
    energy = float(np.sqrt((e * Ke).sum() / (xs * Kx).sum()))
    _report("loose tau=%.0e then resumed sr=%d" % (tau, sr), res, worst,
            "| loose stop at %d iterations, true relative energy error %.3e (tau %.0e; not asserted)" % (res["loose_cg_iterations"], energy, tau))


# ---- delta against the long-double Cholesky solution ------------------------------------------------------------------------------------
def _inv_norm2(L, iters=60):
    """|K^-1|_2 by inverse iteration on K's long-double Cholesky factor (at radius 1e12 the smallest eigenvalue lies below a float64
    eigensolver's error)"""
    x = np.random.default_rng(0).standard_normal(L.shape[0]).astype(LD)
    est = LD(0)
    for _ in range(iters):
        x = x / np.sqrt(x @ x)
        y = PH.cholesky_apply(L, x)
        est = np.sqrt(y @ y)
        x = y
    return float(est)


@pytest.mark.parametrize("radius", [1e4, 1e12])
def test_delta_against_long_double_cholesky(radius):
    case = ("delta", _abi.ANGLE_AXIS, "huber", radius)
    _floor_condition(case)
    g, lin, A, sysm = H.step_reference(*case)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    K = _system_matrix(case)
    L = PH.cholesky_factor(K)
    bv = sysm["b"].reshape(-1)
    star = PH.cholesky_apply(L, bv)
    for _ in range(2):   # (kappa(K) reaches 1e12 at radius 1e12: long-double refinement)
        star = star + PH.cholesky_apply(L, bv - K @ star)
    r_star = float(np.sqrt(((bv - K @ star) ** 2).sum()))
    star = star.reshape(n, 3)
    kinv2 = 1.05 * _inv_norm2(L)
    dev = _device(*case[:3])
    runs = [("textbook", TEXTBOOK, dict(PCG, pcg_single_reduction=0)), ("single", SINGLE, dict(PCG, pcg_single_reduction=1)),
            ("dense", _abi.STEP_DENSE, {"dense_cholesky_max_cams": 512})]
    for tag, path, o in runs:
        res = dev.step_check(g["rot"], radius=radius, **o)
        assert res["path"] == path and res["dense_info"] == 0
        worst = {}
        rel, floor = _check_step(res, case, worst)
        Kd, aKd, _ = H.system_apply(lin, sysm, n, ei, ej, res["delta"])
        r = (sysm["b"] - Kd).reshape(-1)
        ck = np.repeat(H.c_row(A["deg"], 16.0), 3)
        pert = float(np.sqrt(np.sum((C0 * U * (aKd.reshape(-1) + np.abs(sysm["b"].reshape(-1))) + ck * U * aKd.reshape(-1)) ** 2)))
        assert r_star <= 1e-3 * pert, (r_star, pert)   # (the reference solution's own error, |K^-1|_2 r_star, is far inside the bound)
        err = float(np.sqrt(((res["delta"].astype(LD) - star) ** 2).sum()))
        worst["delta"] = err / (kinv2 * (float(np.sqrt(r @ r)) + pert))
        if path == _abi.STEP_DENSE:
            assert res["cg_iterations"] == 0 and res["graph_launches"] > 0
        _report("delta graph %s r=%.0e" % (tag, radius), res, worst, "| |delta - delta*|_2 %.2e, |delta*|_2 %.2e" % (err, float(np.sqrt((star ** 2).sum()))))
    dev.close()
