"""High-precision reference of the per-edge rotation covariance K7 (`k_cov_estimate`, cov_kernels.hpp) (test helper, not a conftest).

Tier 1 (mpmath, 40 digits, per match): the SIGNED Sampson residual s = num / sqrt(den) with the reference's meaning
(src/uncertainty.cpp:36-81, F = K2^-T R [t]x K1^-1), from the double inputs taken exactly and the exact Rodrigues formula (no switch);
r = |s|.  H = sum j j^T and g = sum j r = sum ds s do not depend on the sign, so the reference uses s throughout, which also defines
the value at num == 0 as the one-sided limit.  The Jacobian in the reference's own five parameters by central differences,
h = 1e-18: the rotation as an additive angle-axis (3 columns) and the translation through Ceres 1.14's
HomogeneousVectorParameterization (2 columns), restated below with its `sigma <= DBL_EPSILON` branch decided on the double
fl(x0 x0 + x1 x1).  On that branch Plus(x, d) tends to |x| H e_z, not x, as d -> 0 (Ceres' ComputeHouseholderVector then works on
the unnormalised x); Ceres' Jacobian is the ambient gradient AT x times ComputeJacobian(x), so the differences are taken of
s(x + Plus(x, d) - |x| H e_z), the chart moved to pass through x -- off the branch that is Plus itself.

Tier 2 (numpy longdouble, vectorised over matches; mpmath on the 3 x 3 blocks): per edge the cost, the 5 x 5 H, g, the
elementwise magnitude M = sum |j||j|^T and the per-match evaluation scale of a double j (`jscale`, see edge_data); the rotation
block H_R, its exact inverse C*, kappa_2(H_R) and the pivots of the diagonally pivoted Cholesky (`sym3_rank_deficient`); and one
Levenberg-Marquardt iteration exactly as `k_cov_estimate` runs its first one (lm_step).
"""
import mpmath
import numpy as np

from hp_reference import LD, U, _mp, allowed_relative, ratio  # noqa: F401  (re-exported for the tests)

MP_DPS = 40
FD_H = mpmath.mpf("1e-18")
DBL_EPS = np.finfo(np.float64).eps


def _ld(x):
    return LD(mpmath.nstr(x, 25))


# ---- the rotation (exact Rodrigues) and the chart, in mpmath ----
def rodrigues(w):
    t2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if t2 == 0:
        return [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    t = mpmath.sqrt(t2)
    k = [x / t for x in w]
    s, c = mpmath.sin(t), mpmath.cos(t)
    K = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    KK = [[sum(K[i][m] * K[m][j] for m in range(3)) for j in range(3)] for i in range(3)]
    return [[(1 if i == j else 0) + s * K[i][j] + (1 - c) * KK[i][j] for j in range(3)] for i in range(3)]


def householder(x):
    """Ceres internal::ComputeHouseholderVector on the 3-vector x (mpmath), the branch decided on the double fl(x0 x0 + x1 x1)."""
    xf = [float(v) for v in x]
    sigma_d = xf[0] * xf[0] + xf[1] * xf[1]
    v = [x[0], x[1], mpmath.mpf(1)]
    if sigma_d <= DBL_EPS:
        return v, mpmath.mpf(2 if xf[2] < 0 else 0), True
    sigma = x[0] ** 2 + x[1] ** 2
    mu = mpmath.sqrt(x[2] ** 2 + sigma)
    vp = x[2] - mu if x[2] <= 0 else -sigma / (x[2] + mu)
    beta = 2 * vp * vp / (sigma + vp * vp)
    return [x[0] / vp, x[1] / vp, mpmath.mpf(1)], beta, False


def branch_exact_agrees(x):
    """Does the double decision of the pole branch agree with the exact one (sigma <= DBL_EPSILON in exact arithmetic)?"""
    with mpmath.workdps(MP_DPS):
        s = _mp(x[0]) ** 2 + _mp(x[1]) ** 2
        return (float(x[0]) * float(x[0]) + float(x[1]) * float(x[1]) <= DBL_EPS) == (s <= _mp(DBL_EPS))


def _apply_h(v, beta, y):
    vy = v[0] * y[0] + v[1] * y[1] + v[2] * y[2]
    return [y[k] - v[k] * beta * vy for k in range(3)]


def hom_plus(x, d):
    """HomogeneousVectorParameterization::Plus (Ceres 1.14) in mpmath; x, d as mpf lists."""
    nd = mpmath.sqrt(d[0] ** 2 + d[1] ** 2)
    if nd == 0:
        return list(x)
    h = nd / 2
    sbd = mpmath.sin(h) / h
    y = [sbd * d[0] / 2, sbd * d[1] / 2, mpmath.cos(h)]
    v, beta, _ = householder(x)
    nx = mpmath.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
    return [nx * c for c in _apply_h(v, beta, y)]


def hom_plus_local(x, d):
    """The chart moved to pass through x: x + Plus(x, d) - |x| H e_z (equal to Plus off the pole branch); its derivative at 0 is
    Ceres' ComputeJacobian(x) on both sides of the branch."""
    v, beta, _ = householder(x)
    nx = mpmath.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
    o = _apply_h(v, beta, [0, 0, 1])
    p = hom_plus(x, d)
    return [x[k] + p[k] - nx * o[k] for k in range(3)]


def hom_jacobian_fd(x3):
    """The chart's 3 x 2 Jacobian at x by central differences (float), for the CPU check against the oracle."""
    with mpmath.workdps(MP_DPS):
        x = [_mp(v) for v in x3]
        J = np.zeros((3, 2))
        for c in range(2):
            dp = [0, 0]
            dp[c] = FD_H
            dm = [0, 0]
            dm[c] = -FD_H
            p, m = hom_plus_local(x, dp), hom_plus_local(x, dm)
            J[:, c] = [float((p[k] - m[k]) / (2 * FD_H)) for k in range(3)]
        return J


def hom_plus_f(x3, d2):
    with mpmath.workdps(MP_DPS):
        return np.array([float(v) for v in hom_plus([_mp(v) for v in x3], [_mp(v) for v in d2])])


# ---- tier 1: the signed Sampson residual and its Jacobian ----
def _sampson(R, t, p1, p2, f1, f2):
    """s = num / sqrt(den) and the two magnitudes that scale a double evaluation: |p1| |t| |p2| (num's) and sqrt(den)."""
    c = [t[1] * p1[2] - t[2] * p1[1], t[2] * p1[0] - t[0] * p1[2], t[0] * p1[1] - t[1] * p1[0]]
    a = [R[i][0] * c[0] + R[i][1] * c[1] + R[i][2] * c[2] for i in range(3)]
    num = p2[0] * a[0] + p2[1] * a[1] + p2[2] * a[2]
    rp = [R[0][i] * p2[0] + R[1][i] * p2[1] + R[2][i] * p2[2] for i in range(3)]
    b0, b1 = rp[1] * t[2] - rp[2] * t[1], rp[2] * t[0] - rp[0] * t[2]
    den = (b0 / f1) ** 2 + (b1 / f1) ** 2 + (a[0] / f2) ** 2 + (a[1] / f2) ** 2
    return num / mpmath.sqrt(den), den


def _pix(m, K):
    f1, u1, v1, f2, u2, v2 = [_mp(x) for x in K]
    p1 = [(_mp(m[0]) - u1) / f1, (_mp(m[1]) - v1) / f1, mpmath.mpf(1)]
    p2 = [(_mp(m[2]) - u2) / f2, (_mp(m[3]) - v2) / f2, mpmath.mpf(1)]
    return p1, p2, f1, f2


def edge_tier1(matches, K, rot, t, jac=True):
    """Per match of one edge: s (n), the Jacobian (n x 5) and jscale (n), all long double.  jscale = |p1| |t| |p2| / sqrt(den)
    * (1 + |t|^2 (|p1|^2 + |p2|^2) / (min f^2 den)) (2-norms): the magnitude of num's and den's terms, carried through the quotient -- the
    scale of the rounding error of a double s and of each component of a double j (rotation columns: through J_l, |J_l| <= 1.3;
    translation columns: d s / d t scales as 1 / |t|, the chart's Jacobian as |t|)."""
    n = len(matches)
    s = np.zeros(n, LD)
    J = np.zeros((n, 5), LD)
    sc = np.zeros(n, LD)
    with mpmath.workdps(MP_DPS):
        w = [_mp(x) for x in rot]
        tt = [_mp(x) for x in t]
        R0 = rodrigues(w)
        if jac:
            Rpm = []
            for k in range(3):
                wp, wm = list(w), list(w)
                wp[k] += FD_H
                wm[k] -= FD_H
                Rpm.append((rodrigues(wp), rodrigues(wm)))
            Tpm = []
            for c in range(2):
                dp, dm = [0, 0], [0, 0]
                dp[c], dm[c] = FD_H, -FD_H
                Tpm.append((hom_plus_local(tt, dp), hom_plus_local(tt, dm)))
        tn = mpmath.sqrt(sum(x * x for x in tt))
        fmin = min(abs(_mp(K[0])), abs(_mp(K[3])))
        memo = {}   # (an edge may repeat a match: its values are taken once)
        for i, m in enumerate(matches):
            key = tuple(float(x) for x in m)
            if key in memo:
                s[i], J[i], sc[i] = memo[key]
                continue
            p1, p2, f1, f2 = _pix(m, K)
            s0, den = _sampson(R0, tt, p1, p2, f1, f2)
            s[i] = _ld(s0)
            n1, n2 = mpmath.sqrt(sum(x * x for x in p1)), mpmath.sqrt(sum(x * x for x in p2))
            sc[i] = _ld(n1 * tn * n2 / mpmath.sqrt(den) * (1 + tn * tn * (n1 * n1 + n2 * n2) / (fmin * fmin * den)))
            if not jac:
                memo[key] = (s[i], J[i].copy(), sc[i])
                continue
            for k in range(3):
                J[i, k] = _ld((_sampson(Rpm[k][0], tt, p1, p2, f1, f2)[0] - _sampson(Rpm[k][1], tt, p1, p2, f1, f2)[0]) / (2 * FD_H))
            for c in range(2):
                J[i, 3 + c] = _ld((_sampson(R0, Tpm[c][0], p1, p2, f1, f2)[0] - _sampson(R0, Tpm[c][1], p1, p2, f1, f2)[0]) / (2 * FD_H))
            memo[key] = (s[i], J[i].copy(), sc[i])
    return s, J, sc


# ---- tier 2 ----
def sym3_pivots(H3):
    """Pivots of the diagonally pivoted Cholesky of a symmetric 3 x 3 (mpmath, exact from the given entries), in order."""
    A = [[_mp(H3[i][j]) for j in range(3)] for i in range(3)]
    idx = [0, 1, 2]
    piv = []
    for k in range(3):
        best = max(range(k, 3), key=lambda q: A[idx[q]][idx[q]])
        idx[k], idx[best] = idx[best], idx[k]
        p = A[idx[k]][idx[k]]
        piv.append(p)
        if p == 0:
            piv += [mpmath.mpf(0)] * (2 - k)
            break
        for i in range(k + 1, 3):
            for j in range(k + 1, 3):
                A[idx[i]][idx[j]] -= A[idx[i]][idx[k]] * A[idx[k]][idx[j]] / p
    return piv


def edge_data(matches, K, rot, t, jac=True):
    """Everything one edge's bounds need, at the pose (rot, t): tier 1 per match, then the sums in long double.
      cost, H (5 x 5), g (5), M = sum |j||j|^T, Mj = sum jscale (|j| 1^T + 1 |j|^T) (what the Jacobian's own error adds to dH),
      G = sum |j| |s|, Gj = sum jscale (|s| + |j|) (the same for g), cost_mag = sum s^2 / 2 + jscale |s|;
      with jac: HR (3 x 3), C* (its inverse, long double from mpmath), kappa_2(H_R), the pivots and their ratio min(p2, p3) / p1."""
    with mpmath.workdps(MP_DPS):
        s, J, sc = edge_tier1(matches, K, rot, t, jac)
    out = {"s": s, "J": J, "jscale": sc, "cost": LD(0.5) * (s * s).sum(), "cost_mag": (LD(0.5) * s * s + sc * np.abs(s)).sum()}
    if not jac:
        return out
    aJ, aS = np.abs(J), np.abs(s)
    out.update(H=J.T @ J, g=J.T @ s, M=aJ.T @ aJ, Mj=(sc[:, None] * aJ).sum(axis=0)[:, None] + (sc[:, None] * aJ).sum(axis=0)[None, :],
               G=aJ.T @ aS, Gj=(sc[:, None] * (aS[:, None] + aJ)).sum(axis=0))
    HR = out["H"][:3, :3]
    with mpmath.workdps(MP_DPS):
        Hm = mpmath.matrix([[_mp_ld(HR[i, j]) for j in range(3)] for i in range(3)])
        piv = sym3_pivots([[Hm[i, j] for j in range(3)] for i in range(3)])
        out["pivots"] = [float(p) for p in piv]
        out["pivot_ratio"] = float(min(piv[1], piv[2]) / piv[0]) if piv[0] > 0 else 0.0
        if min(piv) > 0:
            C = Hm ** -1
            out["C"] = np.array([[_ld(C[i, j]) for j in range(3)] for i in range(3)])
            ev = mpmath.eigsy(Hm)[0]
            out["kappa"] = float(max(ev) / min(ev))
        else:
            out["C"], out["kappa"] = None, np.inf
    return out


def _mp_ld(x):
    """A long double taken exactly into mpmath."""
    m, e = np.frexp(LD(x))
    return mpmath.ldexp(mpmath.mpf(int(LD(m) * LD(2) ** 64)), int(e) - 64)


def lm_step(matches, K, rot, t, ed):
    """The first LM iteration of k_cov_estimate (radius 1e4) from the tier-2 data `ed` at (rot, t), in long double / mpmath:
    scale, D^2, the scaled damped system (Hs, bs, dd), its solution y (step = -y), delta = S step, the candidate pose (the chart's
    Plus), its cost, the model cost change and the three decisions with their margins."""
    H, g = ed["H"], ed["g"]
    S = LD(1) / (LD(1) + np.sqrt(np.diagonal(H)))
    Hs = S[:, None] * H * S[None, :]
    bs = S * g
    dd = np.clip(np.diagonal(Hs), LD(1e-6), LD(1e32)) / LD(1e4)
    A = Hs + np.diag(dd)
    y = _solve_ld(A, bs)
    step = -y
    delta = S * step
    with mpmath.workdps(MP_DPS):
        crot = [_mp(rot[k]) + _mp_ld(delta[k]) for k in range(3)]
        ct = hom_plus([_mp(v) for v in t], [_mp_ld(delta[3]), _mp_ld(delta[4])])
        crot_ld = np.array([_ld(v) for v in crot])
        ct_ld = np.array([_ld(v) for v in ct])
        sn = mpmath.sqrt(sum((crot[k] - _mp(rot[k])) ** 2 + (ct[k] - _mp(t[k])) ** 2 for k in range(3)))
        x_norm = mpmath.sqrt(sum(_mp(rot[k]) ** 2 + _mp(t[k]) ** 2 for k in range(3)))
    # the candidate's cost: tier 1 at the candidate rounded to double (the device evaluates its own rounded candidate)
    cand = edge_data(matches, K, crot_ld.astype(float), ct_ld.astype(float), jac=False)
    mcc = -(step @ bs) - LD(0.5) * (step @ Hs @ step)
    cost = ed["cost"]
    cost_change = cost - cand["cost"]
    rel_dec = cost_change / mcc
    ptol = float(sn) / (1e-8 * (float(x_norm) + 1e-8))
    out = {"S": S, "Hs": Hs, "bs": bs, "dd": dd, "A": A, "y": y, "delta": delta, "crot": crot_ld, "ct": ct_ld,
           "cand_cost": cand["cost"], "model_cost_change": mcc, "cost_change": cost_change, "rel_dec": rel_dec,
           "param_stop": ptol <= 1.0, "param_margin": ptol,
           "func_stop": abs(cost_change) <= LD(1e-6) * cost, "func_margin": float(abs(cost_change) / (LD(1e-6) * cost)),
           "accept": bool(rel_dec > LD(1e-3)), "rel_dec_margin": float(rel_dec / LD(1e-3))}
    return out


def _solve_ld(A, b):
    """Solve the 5 x 5 system given in long double exactly (mpmath), rounded to long double."""
    with mpmath.workdps(MP_DPS):
        Am = mpmath.matrix([[_mp_ld(A[i, j]) for j in range(len(b))] for i in range(len(b))])
        bm = mpmath.matrix([_mp_ld(v) for v in b])
        xm = mpmath.lu_solve(Am, bm)
        return np.array([_ld(xm[i]) for i in range(len(b))])


# ---- edges for the tests ----
def aa(theta, axis):
    axis = np.asarray(axis, float)
    return theta * axis / np.linalg.norm(axis)


def make_edge(seed, n, rot=None, t=None, noise_px=0.5, f=(1000.0, 1200.0), pp=(480.0, 360.0, 520.0, 400.0), pose_noise=(0.01, 0.02),
              max_px=1e4):
    """One synthetic view pair under x2^T K2^-T R [t]x K1^-1 x1 = 0 (covariance.make_two_view_batch's convention): points in front
    of camera 1, X2 = R (X1 + t), pixel coordinates kept within max_px.  Returns (matches (n x 4), K (6), rot0, t0): the pose the
    kernel starts from, the true one perturbed by pose_noise (rotation, translation direction); pose_noise None keeps the true pose."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rot = rng.uniform(-0.4, 0.4, 3) if rot is None else np.asarray(rot, float)
    t = (lambda v: v / np.linalg.norm(v))(rng.standard_normal(3)) if t is None else np.asarray(t, float)
    f1, f2 = f
    u1, v1, u2, v2 = pp
    Rm = np.array([[float(x) for x in row] for row in rodrigues([_mp(x) for x in rot])])
    tn = np.linalg.norm(t)
    out = []
    while len(out) < n:
        X1 = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(4, 9)]) * tn
        X2 = Rm @ (X1 + t)
        if abs(X2[2]) < 0.5 * tn:
            continue
        m = np.array([f1 * X1[0] / X1[2] + u1, f1 * X1[1] / X1[2] + v1, f2 * X2[0] / X2[2] + u2, f2 * X2[1] / X2[2] + v2])
        m = m + noise_px * rng.standard_normal(4)
        if np.all(np.abs(m) <= max_px):
            out.append(m)
    r0, t0 = rot.copy(), t.copy()
    if pose_noise is not None:
        r0 = rot + pose_noise[0] * rng.standard_normal(3)
        t0 = t + pose_noise[1] * tn * rng.standard_normal(3)
    return np.array(out), np.array([f1, u1, v1, f2, u2, v2]), r0, t0


def batch(edges):
    """[(matches, K, rot, t), ...] -> the flat arrays of covariance.estimate_rotation_covariances."""
    ptr = np.zeros(len(edges) + 1, np.uint64)
    for e, ed in enumerate(edges):
        ptr[e + 1] = ptr[e] + len(ed[0])
    ms = [np.asarray(ed[0], float).reshape(-1, 4) for ed in edges]
    return {"match_ptr": ptr, "matches": np.ascontiguousarray(np.vstack(ms)) if ms else np.zeros((0, 4)),
            "intrinsics": np.array([ed[1] for ed in edges], float).reshape(-1, 6), "rot": np.array([ed[2] for ed in edges], float).reshape(-1, 3),
            "trans": np.array([ed[3] for ed in edges], float).reshape(-1, 3)}


# ---- bounds (first order in u; constants chosen by the tests) ----
def dH_bound(ed, c_h, c_j):
    """componentwise bound on a double H (5 x 5): c_h u M + c_j u Mj"""
    return U * (c_h * ed["M"] + c_j * ed["Mj"])


def cov_bound(ed, c_h, c_j, c_inv):
    """|C_dev - C*| <= (|C*| dH_R |C*|) / (1 - eta) + c_inv u kappa(H_R) max|C*|,  eta = ||C*||_2 ||dH_R||_F; None where eta >= 1/2
    (there a perturbation of H_R within its bound may move C by as much as C itself)"""
    C = ed["C"]
    dH = dH_bound(ed, c_h, c_j)[:3, :3]
    aC = np.abs(C)
    eta = float(np.linalg.norm(C.astype(float), 2) * np.linalg.norm(dH.astype(float)))
    if not eta < 0.5:
        return None
    return aC @ dH @ aC / LD(1 - eta) + c_inv * U * ed["kappa"] * aC.max()
