"""-m gpu: residuals, loss, gradient, diagonal blocks and normal mat-vec of every linearisation path against the high-precision
reference (tests/hp_reference.py) at the branch points of the device's closed forms, with componentwise bounds.

Bounds (u = 2^-53, no maximum over an array anywhere):
  residual r:   |r_dev - r*| <= c u (|W| (1 + |e|) + C_WHITEN kappa(Sigma) ||W||_F |e|_1)   per component (e_mag)
  s:            |s_dev - s*| <= c u (s* + 2 |r*|^T e_mag) + (c u)^2 |e_mag|^2
  rho, rho':    |rho_dev - rho*| <= c u (scale(rho) + rho' * sbound),  |rho'_dev - rho'*| <= c u (rho' + |rho''| sbound)
  gradient:     |g_dev - g*| <= c_k u sum_e |J~_e|^T |r~_e|
  blocks:       |D_dev - D*| <= c_k u sum_e |J~_e|^T |J~_e|
  mat-vec:      |y_dev - y*| <= c_k u sum_e |J~_e|^T |J~_e| |v|
to first order: each |J~|, |r~| above stands for "true magnitude + first-order error scale" in one factor and the true magnitude in
the other (|J~| + dJ)^T |r~| + |J~|^T dr, never a product of two error scales.  |J~| is the unfused magnitude of the corrected Jacobian
sqrt(rho') (|J| + |alpha/s| |r| |r|^T |J|); dJ, dr carry the whitening's own error (C_WHITEN kappa(Sigma) ||W||_F |W^-1 J|, Cholesky whitening
only) and the residual's rounding into the alpha term (hp_reference.corrected).  Each test also asserts that the bounds bind: the median
row's bound allows at most 1e-11 relative error on its true magnitude sum.  c = 64 covers the per-edge chain: the device forms a residual and its Jacobian in ~30 dependent
roundings (two quaternion products, the log or its series, the Jacobian's 3 x 3 products, the whitening, the Corrector), each of
relative size <= u on magnitudes the unfused sums bound.  The assembled quantities take c_k = 16 + deg(k): the unfused magnitude
sums already over-count those roundings' reach (observed worst ratio 0.03 at c = 64), and deg(k) adds the recursive-summation term of row k (Higham:
n - 1 additions, whatever the order).  A series switch that leaves a truncation error of 1e-13 at the switch point breaks the
bound by two orders of magnitude.
"""

import numpy as np
import pytest

from globalsfmpy_amd import _abi
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem

import hp_reference as H

pytestmark = pytest.mark.gpu

U = H.U
C0 = 64.0    # per-edge quantities (residual, s, rho)
ALLOW_MEDIAN = 1e-11   # the median row's bound may allow at most this relative error (kappa = 1e8 rows allow ~1e-6, the whitening's own)
CA = 16.0    # the assembled ones: observed worst ratio 0.03 at c = 64, so c = 16 still leaves 2x headroom and sees a 1e-14 Jacobian error


def _aa(theta, axis):
    axis = np.asarray(axis, float)
    return theta * axis / np.linalg.norm(axis)


def _exp_q(aa):
    t = np.linalg.norm(aa)
    if t == 0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(t / 2)], np.sin(t / 2) * aa / t])


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _log_q(q):
    if q[0] < 0:
        q = -q
    nv = np.linalg.norm(q[1:])
    return q[1:] * 2.0 if nv == 0 else q[1:] * (2 * np.arctan2(nv, q[0]) / nv)


def _rel_for(aa_i, aa_j, e_target):
    """rel_aa such that log(R_j R_i^T R_rel^T) = e_target (up to the double rounding of rel_aa)."""
    qi, qj, qe = _exp_q(np.asarray(aa_i)), _exp_q(np.asarray(aa_j)), _exp_q(np.asarray(e_target))
    qr = _qmul(_qmul(np.array([qe[0], -qe[1], -qe[2], -qe[3]]), qj), np.array([qi[0], -qi[1], -qi[2], -qi[3]]))
    return _log_q(qr)


def branch_graph(seed=7):
    """About 150 cameras: camera parameters at the switches of the device's closed forms, error rotations at theirs, hub rows of degree
    63 / 64 / 65 and > 256, isolated cameras, covariances with kappa 1 / 1e4 / 1e8 and correlations near +-1, inlier weights 0 / 1e-150 / 1."""
    rng = np.random.default_rng(seed)
    n = 150
    rot = np.array([_aa(rng.uniform(0.2, 2.8), rng.standard_normal(3)) for _ in range(n)])
    special = [0.0, 1e-10, 0.1 - 1e-12, 0.1 + 1e-12, 0.1, np.sqrt(0.1), np.pi - 1e-6, np.pi + 1e-6, 4.5, 2 * np.pi - 1e-3]
    for k, t in enumerate(special):
        rot[4 + k] = _aa(t, rng.standard_normal(3)) if t > 0 else 0.0
    rot[20] = [0.3, 1e-300, 0.2]     # QUATERNION_NORM: y of q_j at +-tiny and -0.0
    rot[21] = [0.3, -1e-300, -0.2]
    rot[22] = [0.3, -0.0, 0.4]
    isolated = set(range(140, 150))   # (140-145 then take three lone pairs: a diagonal block of one edge)
    thetas = [0.0, 1e-12, 1e-8, np.sqrt(0.1) - 1e-12, np.sqrt(0.1) + 1e-12, 1.0, 2.0, 3.0, np.pi - 1e-4, np.pi - 1e-7, np.pi - 1e-9,
              0.49, 0.51, 0.02, 0.3, 0.40, 0.42, 0.44]   # (theta^2 0.16-0.19: the series of J_l^-1 must reach there)
    ei, ej, rel = [], [], []
    live = [c for c in range(n) if c not in isolated]

    def add(i, j, theta=None):
        if theta is None:
            theta = thetas[len(ei) % len(thetas)]
        if theta == 0.0 and np.all(rot[i] == 0):
            r = rot[j].copy()   # R_j R_i^T R_rel^T = I exactly
        else:
            r = _rel_for(rot[i], rot[j], _aa(theta, rng.standard_normal(3)) if theta > 0 else np.zeros(3))
        ei.append(i); ej.append(j); rel.append(r)

    for d, hub in ((300, 0), (63, 1), (64, 2), (65, 3)):
        for k in range(d):
            m = live[4 + (k * 7) % (len(live) - 4)]
            if m == hub:
                m = live[-1]
            (add(hub, m) if k % 2 else add(m, hub))
    for c in live[4:]:
        add(c, 4, 0.0) if c != 4 else None   # camera 4 has omega = 0: exact zero error rotations
        add(c, live[(live.index(c) + 1) % len(live)])
    for k, t in enumerate((0.42, 0.43, 0.44)):   # theta^2 0.18-0.19 on a lone pair: the J_l^-1 series' truncation is not diluted by a row sum
        add(140 + 2 * k, 141 + 2 * k, t)
    E = len(ei)
    cov6 = np.empty((E, 6))
    for e in range(E):
        kind = 2 if e % 32 == 5 else 3 if e % 32 == 21 else 1 if e % 32 == 13 else 0   # (kappa 1e4, 1e8 and the near-singular
        # correlations on one edge in 32 each, so that most rows have none: their bounds must bind at the u level, not at kappa u)
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = [(1, 1, 1), (1, 1e-2, 1e-4), (1, 1e-4, 1e-8), None][kind]
        if lam is None:   # correlation near +-1
            rho = (1 - 1e-6) * (1 if e % 64 == 21 else -1)
            S = np.array([[1, rho, 0], [rho, 1, 0], [0, 0, 0.5]])
            S = Q @ S @ Q.T
        else:
            S = Q @ np.diag(lam) @ Q.T
        S *= 1e-8
        cov6[e] = [S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2]]
    w = np.ones(E)
    w[::11] = 0.0
    big = [e for e in range(E) if thetas[e % len(thetas)] >= 1.0]
    w[big[::5]] = 1e-150
    return {"n_cams": n, "edge_i": np.array(ei), "edge_j": np.array(ej), "rel_aa": np.array(rel), "cov6": cov6, "inlier_weight": w, "rot": rot}


@pytest.fixture(scope="module")
def graph():
    return branch_graph()


_REF = {}


def graph_for(g, et):
    """QUATERNION_NORM: without the edges whose q_rel * q_i has |y| < 1e-12 (the canonicalisation's discontinuity: there the sign of a
    rounded y picks the branch, and finite differences and a correct kernel legitimately disagree).  q_j's y of +-1e-300 and -0.0 is
    exact in its input and stays."""
    if et != _abi.QUATERNION_NORM:
        return g
    keep = np.array([abs(_qmul(_exp_q(r), _exp_q(g["rot"][i]))[2]) >= 1e-12 for r, i in zip(g["rel_aa"], g["edge_i"])])
    h = dict(g)
    for k in ("edge_i", "edge_j", "rel_aa", "cov6", "inlier_weight"):
        h[k] = g[k][keep]
    return h


def reference(g, et):
    if et not in _REF:
        _REF[et] = H.edge_set(et, g["edge_i"], g["edge_j"], g["rel_aa"], g["rot"], g["cov6"], g["inlier_weight"])
    return _REF[et]


LOSSES = {
    "none": (None, None, ()),
    "huber": (LF.HuberLoss(0.5), "huber", (0.5,)),
    "softl1": (LF.SoftLOneLoss(0.3), "softl1", (0.3,)),
    "tolerant": (LF.TolerantLoss(0.05, 0.01), "tolerant", (0.05, 0.01)),
    "scaled": (LF.ScaledLoss(LF.HuberLoss(0.5), 2.5), "scaled", (("huber", (0.5,)), 2.5)),
}


def _check_all(g, et, lname, report, callback=False, make=RotationProblem):
    loss, kind, params = LOSSES[lname]
    g = graph_for(g, et)
    ref = reference(g, et)
    lin = H.corrected(ref, kind, params)
    if kind in ("huber", "scaled"):   # no edge within 1e-9 of the Huber knee: finite differences and a kernel may disagree there
        a2 = 0.25
        assert np.all(np.abs(lin["s"].astype(float) - a2) > 1e-9 * a2)
    dev = make(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"], inlier_weight=g["inlier_weight"])
    if callback:
        dev.set_loss_callback(loss.Evaluate)
    else:
        dev.set_loss(loss)
    rd = dev.residuals(g["rot"], want_residuals=True)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    emag = ref["e_mag"]
    rb = C0 * U * emag
    worst = {"r": H.ratio(rd["residuals"], ref["r"], rb)}
    sb = C0 * U * (lin["s"] + 2 * (np.abs(ref["r"]) * emag).sum(axis=1)) + ((C0 * U * emag) ** 2).sum(axis=1)   # (|r| + dr)^2
    worst["s"] = H.ratio(rd["s"], lin["s"], sb)
    rho0, rho1, rho2 = lin["rho"]
    worst["rho"] = H.ratio(rd["rho"][:, 0], rho0, C0 * U * lin["rho_scale"] + rho1 * sb)
    if not callback:   # (a host callback hands back the Python formula's rho' unchanged)
        worst["rho1"] = H.ratio(rd["rho"][:, 1], rho1, C0 * U * rho1 + np.abs(rho2) * sb)
    cost_bound = 0.5 * ((C0 + len(ei)) * U * lin["rho_scale"] + rho1 * sb).sum()
    worst["cost"] = H.ratio(rd["cost"], H.LD(0.5) * rho0.sum(), cost_bound)
    A = H.assemble(lin, n, ei, ej)
    ck = H.c_row(A["deg"], CA)
    ld = dev.linearize(g["rot"])
    bounds = {"g": (ck[:, None] * U * A["g_mag"], A["g_true"]), "D": (ck[:, None, None] * U * A["D_mag"], A["D_true"])}
    worst["g"] = H.ratio(ld["gradient"], A["g"], bounds["g"][0])
    worst["D"] = H.ratio(ld["diag_blocks"], A["D"], bounds["D"][0])
    rng = np.random.default_rng(3)
    for name, v in (("mv_unit", np.eye(3)[np.arange(n) % 3]), ("mv_rand", rng.standard_normal((n, 3)))):
        y, ym, yt = H.matvec(lin, n, ei, ej, v)
        bounds[name] = (ck[:, None] * U * ym, yt)
        worst[name] = H.ratio(dev.normal_matvec(v), y, bounds[name][0])
    dev.close()
    # the bounds must bind: per row, the relative error they allow (bound over the row's true magnitude sum, no error scale in it)
    allow = {k: H.allowed_relative(b, t) for k, (b, t) in bounds.items()}
    report.append((et, lname, worst, allow))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    print("et %d %-9s %s | allowed rel. median %s" % (et, lname, " ".join("%s %.2e" % kv for kv in worst.items()),
                                                     " ".join("%s %.1e" % (k, a) for k, a in allow.items())))
    assert not bad, (et, lname, worst)
    loose = {k: a for k, a in allow.items() if not a <= ALLOW_MEDIAN}
    assert not loose, ("vacuous bound", et, lname, loose)


_LOSS_FOR_TYPE = ["none", "huber", "softl1", "tolerant"]


@pytest.mark.parametrize("et", list(range(9)))
def test_default_path_against_hp_reference(graph, et):
    report = []
    for lname in _LOSS_FOR_TYPE:
        _check_all(graph, et, lname, report)


# the linearisation paths, forced with the create-time switches
PATHS = {
    "k2_general": {"GSFM_K2_FAST": "0"},
    "k_lin3_general": {"GSFM_LAPLACIAN": "0"},
    "k2c": {"GSFM_K3_COLSORT": "1"},
    "k2c_general": {"GSFM_K3_COLSORT": "1", "GSFM_K2_FAST": "0"},
    "k2c_k16": {"GSFM_K3_COLSORT": "1", "GSFM_K3C_K16": "1"},
    "qrel3": {"GSFM_QREL3": "1"},
    "row_lanes_1": {"GSFM_ROW_LANES": "1"},
    "row_lanes_64": {"GSFM_ROW_LANES": "64"},
}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("et", [_abi.ANGLE_AXIS, _abi.ANGLE_AXIS_COVARIANCE, _abi.QUATERNION_COSINE, _abi.ANGLE_AXIS_COV_INLIERS])
def test_forced_paths_against_hp_reference(graph, monkeypatch, path, et):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    report = []
    for lname in ("none", "huber", "tolerant"):
        _check_all(graph, et, lname, report)


@pytest.mark.parametrize("et", [_abi.ANGLE_AXIS, _abi.ANGLE_AXIS_COVARIANCE])
def test_program_and_callback_losses_against_hp_reference(graph, et):
    report = []
    _check_all(graph, et, "scaled", report)
    _check_all(graph, et, "tolerant", report, callback=True)
