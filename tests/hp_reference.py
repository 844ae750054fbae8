"""High-precision reference of the per-edge linearisation and its assembly (test helper, not a conftest).

Tier 1 (mpmath, 40 digits, per edge): the residual of all nine error types with the reference's semantics, the whitening of
1e8 * Sigma and the scalar weights, and the Jacobians in the reference's own parameters (angle-axis: additive; quaternion
types: the 3-dimensional EigenQuaternionParameterization tangent) by central differences with h = 1e-18.  Finite differences
depend on no closed form of either the device or the CPU oracle.  The error rotation's log is taken through the quaternion
(angle 2 atan2(|v|, |w|), in [0, pi]), which is the rotation-matrix log of the reference away from theta = pi.

Tier 2 (numpy longdouble, vectorised): the analytic losses (rho, rho', rho''), the Ceres Corrector and the assembly that
the device performs -- g = sum J~^T r~, the diagonal blocks, the normal mat-vec, the dense damped system, 1/2 sum rho --
from the tier-1 per-edge residuals and Jacobians, together with componentwise magnitudes from which the tests derive
their error bounds (no maximum over an array anywhere).
"""
import mpmath
import numpy as np

from globalsfmpy_amd import _abi

MP_DPS = 40
FD_H = mpmath.mpf("1e-18")
U = 2.0 ** -53   # unit roundoff of fp64
LD = np.longdouble
# the whitening W = L^T, L L^T = inverse(1e8 Sigma), as the reference computes it: a cofactor inverse (about 8 roundings per entry of
# P, a relative perturbation of P amplified by kappa) and a 3 x 3 Cholesky factor (3 n^2 = 27 per unit of P's relative perturbation, the
# same kappa not applied twice to first order): ||dW||_F <= C_WHITEN kappa u ||W||_F with C_WHITEN = 8 * 8, rounded to a power of two
C_WHITEN = 64.0

AA_TYPES = (_abi.ANGLE_AXIS_COVARIANCE, _abi.ANGLE_AXIS, _abi.ANGLE_AXIS_INLIERS, _abi.ANGLE_AXIS_COV_INLIERS,
            _abi.ANGLE_AXIS_COVTRACE, _abi.ANGLE_AXIS_COVNORM)
RES_DIM = {_abi.QUATERNION_NORM: 4, _abi.ROTATION_MAT_FNORM: 9, _abi.QUATERNION_COSINE: 3}


def res_dim(et):
    return RES_DIM.get(et, 3)


# ---- quaternions (w, x, y, z) in mpmath ----
def _mp(x):
    return mpmath.mpf(float(x))


def q_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


def q_conj(a):
    return (a[0], -a[1], -a[2], -a[3])


def aa_to_q(aa):
    """Ceres AngleAxisToQuaternion in exact arithmetic (the input doubles taken exactly)."""
    a = [x if isinstance(x, mpmath.mpf) else _mp(x) for x in aa]
    t2 = a[0] ** 2 + a[1] ** 2 + a[2] ** 2
    if t2 == 0:
        return (mpmath.mpf(1), a[0] / 2, a[1] / 2, a[2] / 2)
    t = mpmath.sqrt(t2)
    k = mpmath.sin(t / 2) / t
    return (mpmath.cos(t / 2), k * a[0], k * a[1], k * a[2])


def q_log(q):
    """Angle-axis of a unit quaternion, angle in [0, pi] (double cover folded)."""
    w, v = q[0], q[1:]
    if w < 0:
        w, v = -w, tuple(-x for x in v)
    nv = mpmath.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    if nv == 0:
        return [2 * x / w for x in v]
    k = 2 * mpmath.atan2(nv, w) / nv
    return [k * x for x in v]


def q_to_mat(q):
    w, x, y, z = q
    n = w * w + x * x + y * y + z * z
    return [[(w * w + x * x - y * y - z * z) / n, 2 * (x * y - w * z) / n, 2 * (x * z + w * y) / n],
            [2 * (x * y + w * z) / n, (w * w - x * x + y * y - z * z) / n, 2 * (y * z - w * x) / n],
            [2 * (x * z - w * y) / n, 2 * (y * z + w * x) / n, (w * w - x * x - y * y + z * z) / n]]


def q_plus(q, d):
    """EigenQuaternionParameterization::Plus: Exp(d) (not halved) times q."""
    nd = mpmath.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
    if nd == 0:
        return q
    k = mpmath.sin(nd) / nd
    return q_mul((mpmath.cos(nd), k * d[0], k * d[1], k * d[2]), q)


# ---- whitening (the reference: 1e8 * Sigma, W = L^T with L L^T = inverse) ----
def whitening(et, cov6=None, inlier_w=1.0):
    """3x3 mpmath matrix W (row-major lists) and the condition number that scales W's own rounding error: kappa(Sigma) for the
    Cholesky whitening (inverse, then factor), 1 for every scalar weight."""
    one = mpmath.mpf(1)
    eye = lambda w: [[w, 0, 0], [0, w, 0], [0, 0, w]]
    if et in (_abi.ANGLE_AXIS, _abi.QUATERNION_NORM, _abi.QUATERNION_COSINE, _abi.ROTATION_MAT_FNORM):
        return eye(one), 1.0
    if et == _abi.ANGLE_AXIS_INLIERS:
        return eye(_mp(inlier_w)), 1.0
    c = [_mp(x) * mpmath.mpf(10) ** 8 for x in cov6]
    S = mpmath.matrix([[c[0], c[3], c[4]], [c[3], c[1], c[5]], [c[4], c[5], c[2]]])
    ev = mpmath.eigsy(S)[0]
    kappa = float(max(abs(e) for e in ev) / min(abs(e) for e in ev))
    # a scalar weight from the trace or the Frobenius norm is as accurate as its few roundings, whatever kappa(Sigma): kappa 1
    if et == _abi.ANGLE_AXIS_COVTRACE:
        return eye(mpmath.sqrt(one / (c[0] + c[1] + c[2]))), 1.0
    if et == _abi.ANGLE_AXIS_COVNORM:
        f = sum(S[i, j] ** 2 for i in range(3) for j in range(3))
        return eye(mpmath.sqrt(one / mpmath.sqrt(f))), 1.0
    L = mpmath.cholesky(S ** -1)
    w = _mp(inlier_w) if et == _abi.ANGLE_AXIS_COV_INLIERS else one
    return [[L[j, i] * w for j in range(3)] for i in range(3)], kappa


# ---- tier 1: one edge ----
class Edge1(object):
    """One edge's residual function of the 6 local parameters (delta_i, delta_j) in the reference's parameterisation."""

    def __init__(self, et, aa_i, aa_j, rel_aa, W):
        self.et, self.W = et, W
        self.aa_i = [_mp(x) for x in aa_i]
        self.aa_j = [_mp(x) for x in aa_j]
        self.qr = aa_to_q(rel_aa)
        if et not in AA_TYPES:
            self.qi, self.qj = aa_to_q(aa_i), aa_to_q(aa_j)
        self.signs = None
        if et == _abi.QUATERNION_NORM:   # the canonicalisation's branch at the point itself; the derivatives are the branch's
            est = q_mul(self.qr, self.qi)
            self.signs = (-1 if self.qj[2] < 0 else 1, -1 if est[2] < 0 else 1)

    def residual(self, d=(0, 0, 0, 0, 0, 0)):
        et, W = self.et, self.W
        if et in AA_TYPES:
            qi = aa_to_q([self.aa_i[k] + d[k] for k in range(3)])
            qj = aa_to_q([self.aa_j[k] + d[3 + k] for k in range(3)])
            e = q_log(q_mul(q_mul(qj, q_conj(qi)), q_conj(self.qr)))   # R_j R_i^T R_rel^T
            return [W[r][0] * e[0] + W[r][1] * e[1] + W[r][2] * e[2] for r in range(3)]
        qi, qj = q_plus(self.qi, d[:3]), q_plus(self.qj, d[3:])
        if et == _abi.QUATERNION_COSINE:
            dq = q_mul(self.qr, q_conj(q_mul(qj, q_conj(qi))))
            return [2 * dq[1], 2 * dq[2], 2 * dq[3]]
        if et == _abi.QUATERNION_NORM:
            est = q_mul(self.qr, qi)
            sj, se = self.signs
            return [sj * qj[k] - se * est[k] for k in (1, 2, 3, 0)]   # (x, y, z, w)
        Ri, Rj, Rr = q_to_mat(qi), q_to_mat(qj), q_to_mat(self.qr)
        est = [[sum(Rr[r][k] * Ri[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
        return [est[k % 3][k // 3] - Rj[k % 3][k // 3] for k in range(9)]   # column-major

    def error_angle(self):
        e = q_log(q_mul(q_mul(aa_to_q(self.aa_j), q_conj(aa_to_q(self.aa_i))), q_conj(self.qr)))
        return mpmath.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)

    def linearise(self):
        """(r, Ji, Jj) as mpmath lists: R, R x 3, R x 3."""
        r = self.residual()
        J = [[None] * 6 for _ in r]
        for p in range(6):
            dp = [0] * 6
            dm = [0] * 6
            dp[p], dm[p] = FD_H, -FD_H
            rp, rm = self.residual(dp), self.residual(dm)
            for k in range(len(r)):
                J[k][p] = (rp[k] - rm[k]) / (2 * FD_H)
        return r, [row[:3] for row in J], [row[3:] for row in J]


def edge_set(et, edge_i, edge_j, rel_aa, rot_aa, cov6=None, inlier_weight=None):
    """Tier 1 for every edge, as long-double arrays: r (E x R), Ji, Jj (E x R x 3), and the first-order error scales a double
    evaluation carries (each to be multiplied by c u):
      e_mag (E x R):   of the residual -- |W| (1 + |e|) for the rounding of e and W e, plus the whitening's own error
                       |dW e| <= C_WHITEN kappa ||W||_F |e|_1  (||dW||_F <= C_WHITEN kappa u ||W||_F, first order in u)
      Jw_i, Jw_j (E x 3): of the Jacobian's columns through dW:  C_WHITEN kappa ||W||_F sum_k |de_k / dx_c|,  de/dx = W^-1 J
    (zero for the scalar weights, whose relative error is a few u and lies inside c), kappa (E), W (E x 3 x 3, float)."""
    E, R = len(edge_i), res_dim(et)
    out = {"r": np.zeros((E, R), LD), "Ji": np.zeros((E, R, 3), LD), "Jj": np.zeros((E, R, 3), LD),
           "e_mag": np.zeros((E, R), LD), "Jw_i": np.zeros((E, 3), LD), "Jw_j": np.zeros((E, 3), LD),
           "kappa": np.ones(E), "W": np.zeros((E, 3, 3))}
    with mpmath.workdps(MP_DPS):
        for e in range(E):
            W, kappa = whitening(et, None if cov6 is None else cov6[e], 1.0 if inlier_weight is None else inlier_weight[e])
            ed = Edge1(et, rot_aa[edge_i[e]], rot_aa[edge_j[e]], rel_aa[e], W)
            r, Ji, Jj = ed.linearise()
            out["r"][e] = [LD(mpmath.nstr(x, 25)) for x in r]
            out["Ji"][e] = [[LD(mpmath.nstr(x, 25)) for x in row] for row in Ji]
            out["Jj"][e] = [[LD(mpmath.nstr(x, 25)) for x in row] for row in Jj]
            Wf = np.array([[float(W[a][b]) for b in range(3)] for a in range(3)])
            out["W"][e], out["kappa"][e] = Wf, kappa
            if et in AA_TYPES:
                theta = float(ed.error_angle())
                out["e_mag"][e] = np.abs(Wf).sum(axis=1) * (1.0 + theta)
                if kappa > 1.0 and np.any(Wf):   # (an inlier weight of 0 zeroes W, r and J)
                    wf = C_WHITEN * kappa * np.sqrt((Wf * Wf).sum())
                    out["e_mag"][e] += wf * np.abs(np.linalg.solve(Wf, out["r"][e].astype(float))).sum()
                    out["Jw_i"][e] = wf * np.abs(np.linalg.solve(Wf, out["Ji"][e].astype(float))).sum(axis=0)
                    out["Jw_j"][e] = wf * np.abs(np.linalg.solve(Wf, out["Jj"][e].astype(float))).sum(axis=0)
            else:
                out["e_mag"][e] = 1.0
    return out


# ---- tier 2: losses, Corrector, assembly in long double ----
def loss_rho(kind, params, s):
    """(rho, rho', rho'', scale): Ceres' formulas in long double; `scale` is the absolute magnitude of the terms the formula
    adds or subtracts (its own evaluation scale, before cancellation)."""
    s = np.asarray(s, LD)
    one = LD(1)
    if kind is None or kind == "trivial":
        return s, np.ones_like(s), np.zeros_like(s), s
    if kind == "huber":
        a = LD(params[0]); b = a * a
        out = s > b
        root = np.sqrt(np.where(out, s, one))
        d1 = a / root
        return (np.where(out, 2 * a * root - b, s), np.where(out, d1, one), np.where(out, -d1 / (2 * np.where(out, s, one)), 0),
                np.where(out, 2 * a * root + b, s))
    if kind == "softl1":
        a = LD(params[0]); b = a * a; c = one / b
        t = one + s * c; root = np.sqrt(t)
        return 2 * b * (root - 1), one / root, -(c / root) / (2 * t), 2 * b * (root + 1)
    if kind == "cauchy":
        a = LD(params[0]); b = a * a; c = one / b
        t = one + s * c; inv = one / t
        return b * np.log(t), inv, -c * inv * inv, b * (1 + np.abs(np.log(t)))
    if kind == "tolerant":
        a, bb = LD(params[0]), LD(params[1])
        c = bb * np.log(one + np.exp(-a / bb))
        x = (s - a) / bb
        lin = x > LD(36.7)   # the reference's own switch to the linear branch
        xe = np.where(lin, 0, x)
        ex = np.exp(xe)
        rho = np.where(lin, s - a - c, bb * np.log(one + ex) - c)
        return (rho, np.where(lin, one, ex / (one + ex)), np.where(lin, 0, LD(0.5) / (bb * (one + np.cosh(xe)))),
                np.where(lin, s + a + c, bb * (one + np.log(one + ex)) + c))   # (log of a rounded 1 + e^x: absolute error u)
    if kind == "scaled":   # ScaledLoss(inner, k)
        inner, k = params
        r0, r1, r2, sc = loss_rho(inner[0], inner[1], s)
        k = LD(k)
        return k * r0, k * r1, k * r2, k * sc
    raise ValueError(kind)


def corrected(ref, kind=None, params=()):
    """Apply loss + Corrector: adds s, rho (3 x E), r~, Ji~, Jj~ and, for the bounds, first-order magnitudes (each multiplied by c u
    in the tests, never by each other's error scale):
      rt_abs = |r~| and rt_err = residual_scaling * e_mag (the residual's own error);
      Jit_abs = sqrt(rho') (|J| + |alpha/s| |r| |r|^T |J|) (the unfused magnitude, roundings) and Jit_err (what dW and the residual's
      error carry into the Corrector's alpha term)."""
    out = dict(ref)
    r, Ji, Jj = ref["r"], ref["Ji"], ref["Jj"]
    s = (r * r).sum(axis=1)
    rho0, rho1, rho2, scale = loss_rho(kind, params, s)
    sq1 = np.sqrt(rho1)
    full = (s > 0) & (rho2 > 0)
    sd = np.where(full, s, 1)
    alpha = np.where(full, 1 - np.sqrt(np.where(full, 1 + 2 * sd * rho2 / rho1, 1)), 0)
    rs = sq1 / (1 - alpha)
    asn = alpha / sd
    rt = rs[:, None] * r
    out.update(s=s, rho=np.stack([rho0, rho1, rho2]), rho_scale=scale, rt=rt, sqrt_rho1=sq1, residual_scaling=rs,
               rt_abs=np.abs(rt), rt_err=rs[:, None] * ref["e_mag"])
    ar, em, aasn = np.abs(r), ref["e_mag"], np.abs(asn)[:, None, None]
    for side, J, Jw in (("i", Ji, ref["Jw_i"]), ("j", Jj, ref["Jw_j"])):
        rtJ = np.einsum("er,erc->ec", r, J)
        out["J%st" % side] = sq1[:, None, None] * (J - asn[:, None, None] * r[:, :, None] * rtJ[:, None, :])
        aJ = np.abs(J)
        out["J%st_abs" % side] = sq1[:, None, None] * (aJ + aasn * ar[:, :, None] * np.einsum("er,erc->ec", ar, aJ)[:, None, :])
        err = Jw[:, None, :] + aasn * (em[:, :, None] * np.einsum("er,erc->ec", ar, aJ)[:, None, :]
                                       + ar[:, :, None] * np.einsum("er,erc->ec", em, aJ)[:, None, :]
                                       + ar[:, :, None] * np.einsum("er,ec->ec", ar, Jw)[:, None, :])
        out["J%st_err" % side] = sq1[:, None, None] * np.broadcast_to(err, J.shape)
    return out


def assemble(lin, n_cams, edge_i, edge_j):
    """g (n x 3), D (n x 3 x 3), cost, the per-camera degree, and per quantity two magnitude sums: `*_mag`, the first-order bound's
    sum (an error scale times a true magnitude, never two error scales), and `*_true`, the sum of the true magnitudes alone."""
    ei, ej = np.asarray(edge_i), np.asarray(edge_j)
    z3, z33 = (lambda: np.zeros((n_cams, 3), LD)), (lambda: np.zeros((n_cams, 3, 3), LD))
    g, gm, gt, D, Dm, Dt = z3(), z3(), z3(), z33(), z33(), z33()
    for cam, side in ((ei, "i"), (ej, "j")):
        J, Ja, Je = lin["J%st" % side], lin["J%st_abs" % side], lin["J%st_err" % side]
        np.add.at(g, cam, np.einsum("erc,er->ec", J, lin["rt"]))
        np.add.at(gt, cam, np.einsum("erc,er->ec", Ja, lin["rt_abs"]))
        np.add.at(gm, cam, np.einsum("erc,er->ec", Ja + Je, lin["rt_abs"]) + np.einsum("erc,er->ec", Ja, lin["rt_err"]))
        np.add.at(D, cam, np.einsum("era,erb->eab", J, J))
        np.add.at(Dt, cam, np.einsum("era,erb->eab", Ja, Ja))
        np.add.at(Dm, cam, np.einsum("era,erb->eab", Ja + Je, Ja) + np.einsum("era,erb->eab", Ja, Ja + Je))
    deg = np.bincount(ei, minlength=n_cams) + np.bincount(ej, minlength=n_cams)
    return {"g": g, "g_mag": gm, "g_true": gt, "D": D, "D_mag": Dm, "D_true": Dt, "cost": LD(0.5) * lin["rho"][0].sum(), "deg": deg}


def matvec(lin, n_cams, edge_i, edge_j, v):
    """y = J~^T J~ v, its first-order bound's sum (|J~| + dJ)^T |J~| |v| + |J~|^T (|J~| + dJ) |v|, and the true sum |J~|^T |J~| |v|."""
    ei, ej = np.asarray(edge_i), np.asarray(edge_j)
    v = np.asarray(v, LD)
    av = np.abs(v)
    Jv = np.einsum("erc,ec->er", lin["Jit"], v[ei]) + np.einsum("erc,ec->er", lin["Jjt"], v[ej])
    Jva = np.einsum("erc,ec->er", lin["Jit_abs"], av[ei]) + np.einsum("erc,ec->er", lin["Jjt_abs"], av[ej])
    Jve = Jva + np.einsum("erc,ec->er", lin["Jit_err"], av[ei]) + np.einsum("erc,ec->er", lin["Jjt_err"], av[ej])
    y, ym, yt = (np.zeros((n_cams, 3), LD) for _ in range(3))
    for cam, side in ((ei, "i"), (ej, "j")):
        J, Ja, Je = lin["J%st" % side], lin["J%st_abs" % side], lin["J%st_err" % side]
        np.add.at(y, cam, np.einsum("erc,er->ec", J, Jv))
        np.add.at(yt, cam, np.einsum("erc,er->ec", Ja, Jva))
        np.add.at(ym, cam, np.einsum("erc,er->ec", Ja + Je, Jva) + np.einsum("erc,er->ec", Ja, Jve))
    return y, ym, yt


def normal_matrix(lin, n_cams, edge_i, edge_j, key="t"):
    """The dense J~^T J~ (3n x 3n, long double); key "t_abs" gives |J~|^T |J~|."""
    n = 3 * n_cams
    A = np.zeros((n, n), LD)
    for e, (i, j) in enumerate(zip(edge_i, edge_j)):
        Ji, Jj = lin["Ji" + key][e], lin["Jj" + key][e]
        for a, Ja in ((i, Ji), (j, Jj)):
            for b, Jb in ((i, Ji), (j, Jj)):
                A[3 * a:3 * a + 3, 3 * b:3 * b + 3] += Ja.T @ Jb
    return A


def cholesky_solve(A, B):
    """Solve A X = B for symmetric positive definite A in long double (numpy's LAPACK has no long double)."""
    L = np.array(A, LD)
    n = L.shape[0]
    for k in range(n):
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    L = np.tril(L)
    X = np.array(B, LD).reshape(n, -1)
    for k in range(n):   # forward
        X[k] /= L[k, k]
        X[k + 1:] -= np.outer(L[k + 1:, k], X[k])
    for k in range(n - 1, -1, -1):   # backward
        X[k] /= L[k, k]
        X[:k] -= np.outer(L[k, :k], X[k])
    return X.reshape(np.shape(B))


def ratio(dev, ref, bound):
    """Worst |dev - ref| / bound (bound > 0 where it matters; a zero bound demands equality)."""
    err = np.abs(np.asarray(dev, LD) - np.asarray(ref, LD))
    b = np.asarray(bound, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0))
    return float(q.max()) if q.size else 0.0


def allowed_relative(bound, true):
    """Median over the entries with a nonzero true magnitude of bound / true: the relative error a bound lets pass."""
    b, t = np.asarray(bound, float).ravel(), np.asarray(true, float).ravel()
    keep = t > 0
    return float(np.median(b[keep] / t[keep])) if keep.any() else 0.0


def c_row(deg, c0=64):
    """The bound's constant per camera row: c0 roundings per summand (the edge's residual, Jacobian and Corrector chain) plus the
    recursive-summation term (Higham: n - 1 additions of a row's summands, whatever the order and grouping)."""
    return (c0 + np.asarray(deg, float))



# ---- the damped normal system of one LM step, in the reference's parameters (tests/test_hp_step_reference.py, test_gpu_hp_step.py) ----
# The device solves (J^T J + Lambda) eta = -g in its internal tangent eta = T delta and stops PCG on sqrt(r.M^-1 r / b.M^-1 b) with M the
# damped diagonal blocks.  With K* = T^T K_eta T, b* = T^T b_eta, M* = T^T M_eta T and r* = b* - K* delta = T^T r_eta:
#   r*.M*^-1 r* = r_eta^T T (T^-1 M_eta^-1 T^-T) T^T r_eta = r_eta.M_eta^-1 r_eta   (likewise for b),
# so the stopping quantity is the same number here, and a device step delta = T^-1 eta can be judged without knowing T.
def sym3_inverse(M):
    """Inverses of n symmetric 3 x 3 matrices (n x 3 x 3, long double) by cofactors."""
    M = np.asarray(M, LD)
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    out = np.empty_like(M)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00, c01, c02
    out[:, 1, 1], out[:, 1, 2], out[:, 2, 2] = a * f - c * c, b * c - a * e, a * d - b * b
    out[:, 1, 0], out[:, 2, 0], out[:, 2, 1] = out[:, 0, 1], out[:, 0, 2], out[:, 1, 2]
    return out / det[:, None, None]


def damped_system(A, radius, jacobi_scaling=True, min_diag=1e-6, max_diag=1e32):
    """LevenbergMarquardtStrategy's system from assemble()'s output: lam* (n x 3), b* = -g*, the blocks M_k = D*_k + diag(lam*_k) and
    their inverses.  A camera without an edge has D = 0, g = 0: lam = min_diag / radius, b = 0."""
    D = A["D"]
    dd = np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], axis=1)
    sc = 1 / (1 + np.sqrt(dd)) if jacobi_scaling else np.ones_like(dd)
    lam = np.clip(sc * sc * dd, LD(min_diag), LD(max_diag)) / (LD(radius) * sc * sc)
    M = D.copy()
    for c in range(3):
        M[:, c, c] += lam[:, c]
    return {"lam": lam, "b": -A["g"], "M": M, "Minv": sym3_inverse(M), "radius": radius}


def system_apply(lin, sysm, n_cams, edge_i, edge_j, delta):
    """(K* delta, the magnitude sum that bounds |K*| |delta| to first order, H* delta)."""
    delta = np.asarray(delta, LD).reshape(n_cams, 3)
    y, ym, _ = matvec(lin, n_cams, edge_i, edge_j, delta)
    return y + sysm["lam"] * delta, ym + sysm["lam"] * np.abs(delta), y


def mnorm(sysm, z, cams=None):
    """||z||_{M^-1}, over all cameras or the subset `cams`."""
    z = np.asarray(z, LD).reshape(-1, 3)
    Mi = sysm["Minv"]
    if cams is not None:
        z, Mi = z[cams], Mi[cams]
    return np.sqrt(np.einsum("ka,kab,kb->", z, Mi, z))


def step_residual(lin, A, sysm, n_cams, edge_i, edge_j, delta, cams=None, c0=64.0, ca=16.0):
    """The true relative residual of `delta` in the M^-1 norm, sqrt(r.M^-1 r / b.M^-1 b), r = b* - K* delta, and the rounding floor
       || c0 u (|K*||delta| + |b*|) + c_row(deg, ca) u (|K*||delta| + g_mag) ||_{M^-1} / ||b*||_{M^-1}:
    what a double-precision evaluation of r at this delta can be off by -- c0 roundings on the operands' magnitudes (the block's
    products, the subtraction from b), the assembled quantities' own bound (test_gpu_hp_linearization.py: c_k = ca + deg(k) on the
    first-order magnitude sums of the mat-vec and of the gradient).  cams: restrict both norms to a subset (one connected component)."""
    Kd, aKd, _ = system_apply(lin, sysm, n_cams, edge_i, edge_j, delta)
    r = sysm["b"] - Kd
    ck = c_row(A["deg"], ca)[:, None]
    e = c0 * U * (aKd + np.abs(sysm["b"])) + ck * U * (aKd + A["g_mag"])
    bn = mnorm(sysm, sysm["b"], cams)
    return float(mnorm(sysm, r, cams) / bn), float(mnorm(sysm, e, cams) / bn), r


def model_cost_change(lin, A, n_cams, edge_i, edge_j, delta):
    """-delta.g* - 1/2 delta^T H* delta, and the magnitude sum |delta|.|g*| + 1/2 |delta|^T |H*| |delta| of its terms."""
    delta = np.asarray(delta, LD).reshape(n_cams, 3)
    y, ym, _ = matvec(lin, n_cams, edge_i, edge_j, delta)
    ad = np.abs(delta)
    return -(delta * A["g"]).sum() - LD(0.5) * (delta * y).sum(), (ad * (np.abs(A["g"]) + A["g_mag"])).sum() + LD(0.5) * (ad * ym).sum()


def system_matrix(lin, sysm, n_cams, edge_i, edge_j):
    """The dense K* = H* + diag(lam*) (3n x 3n, long double)."""
    K = normal_matrix(lin, n_cams, edge_i, edge_j)
    K[np.diag_indices(3 * n_cams)] += sysm["lam"].reshape(-1)
    return K


def solve_refined(K, b, sweeps=3):
    """K x = b: a float64 LAPACK solve refined with long-double residuals (each sweep gains ~1 / (kappa u) digits)."""
    Kf = np.array(K, float)
    import scipy.linalg as sla
    cf = sla.cho_factor(Kf)
    b = np.asarray(b, LD).reshape(-1)
    x = np.zeros_like(b)
    for _ in range(sweeps + 1):
        x = x + sla.cho_solve(cf, np.array(b - K @ x, float)).astype(LD)
    return x


# ---- the graphs of the step tests --------------------------------------------------------------------------------------------------
def _rel_measured(gt_aa, i, j, noise_aa):
    """rel_aa of edge (i, j): Exp(noise) R_j R_i^T (R_j = R_ij R_i)."""
    from globalsfmpy_amd import synth
    q = synth.aa_to_quat(gt_aa)
    qr = synth.quat_mul(synth.quat_mul(synth.aa_to_quat(noise_aa), q[j]), synth.quat_conj(q[i]))
    return synth.quat_to_aa(qr)


def iso_cov6(n_edges, seed):
    """Per-edge isotropic covariances sigma_e^2 I, sigma_e log-uniform over a decade (0.5 to 5 degrees), scaled as synth.make_graph scales
    its own (3e-4 Sigma): kappa(Sigma) = 1, so the whitening's own error term C_WHITEN kappa u, which puts the step floor of make_graph's
    covariances (kappa up to 96) at 2.3-3.8e-10, vanishes from the bound.  Measured with these on the main graph under Huber(0.5), radius 1e4: floor 1.63e-13 for
    ANGLE_AXIS_COVARIANCE and 1.95e-13 for ANGLE_AXIS_COV_INLIERS (tests/test_hp_step_reference.py prints them)."""
    rng = np.random.default_rng(seed)
    s2 = 3e-4 * np.deg2rad(10.0 ** rng.uniform(np.log10(0.5), np.log10(5.0), n_edges)) ** 2
    c = np.zeros((n_edges, 6))
    c[:, 0] = c[:, 1] = c[:, 2] = s2
    return c


def _with_hubs(g, hubs, seed, noise_deg=1.0):
    """Adds edges from the hub cameras (camera, target degree) to cameras that are not yet their neighbours, alternating the edge's
    orientation, measured from the ground truth with `noise_deg` of noise."""
    rng = np.random.default_rng(seed)
    n = g["n_cams"]
    ei, ej, rel = list(g["edge_i"]), list(g["edge_j"]), list(g["rel_aa"])
    hub_ids = set(h for h, _ in hubs)
    for hub, target in hubs:
        nb = set(j for i, j in zip(ei, ej) if i == hub) | set(i for i, j in zip(ei, ej) if j == hub)
        deg = len([1 for i, j in zip(ei, ej) if hub in (i, j)])
        free = [c for c in range(n) if c not in nb and c not in hub_ids]
        picks = rng.permutation(free)[:target - deg]
        assert len(picks) == target - deg
        for k, m in enumerate(picks):
            i, j = (hub, int(m)) if k % 2 else (int(m), hub)
            ei.append(i); ej.append(j)
            rel.append(_rel_measured(g["gt_aa"], i, j, np.deg2rad(noise_deg) * rng.standard_normal(3)))
    E = len(ei)
    out = dict(g)
    out.update(edge_i=np.array(ei, dtype=np.uint32), edge_j=np.array(ej, dtype=np.uint32), rel_aa=np.array(rel),
               cov6=iso_cov6(E, seed + 1), inlier_weight=np.random.default_rng(seed + 2).uniform(0.2, 3.0, E), rot=g["init_aa"])
    return out


def step_main_graph(seed=11):
    """600 cameras -- three blocks of 256 of the camera kernels, the last partial -- from synth.make_graph(600, 1500) with its init_aa as
    the linearisation point (2 degrees from the ground truth) and hubs of degree 63 / 64 / 65 / 300 on top: about 2000 edges.  A tenth of
    make_graph's non-chain edges are outliers (uniform random rotations), so that Huber(0.5) and the Tolerant loss are on their
    non-trivial branches on some edges."""
    from globalsfmpy_amd import synth
    g = synth.make_graph(600, 1500, seed, outlier_frac=0.1)
    return _with_hubs(g, ((0, 300), (1, 63), (2, 64), (3, 65)), seed)


def step_delta_graph(seed=12):
    """150 cameras (450 unknowns: a long-double Cholesky solve is affordable), one hub of degree 65."""
    from globalsfmpy_amd import synth
    g = synth.make_graph(150, 400, seed, outlier_frac=0.1)
    return _with_hubs(g, ((0, 65),), seed)


def step_two_component_graph(seed=13):
    """A component of 36 cameras (factorised under dense_cholesky_max_cams = 40) beside one of 300 (PCG) and two cameras without an
    edge, interleaved in the numbering.  comp: 0 the large component, 1 the small one, 2 the isolated cameras."""
    from globalsfmpy_amd import synth
    a = _with_hubs(synth.make_graph(300, 800, seed, outlier_frac=0.1), ((0, 65),), seed)
    b = _with_hubs(synth.make_graph(36, 90, seed + 5, outlier_frac=0.1), (), seed + 5)
    n = 338
    ids = np.random.default_rng(seed).permutation(n)
    ia, ib = np.sort(ids[:300]), np.sort(ids[300:336])
    out = {"n_cams": n, "comp": np.full(n, 2)}
    out["comp"][ia], out["comp"][ib] = 0, 1
    out["edge_i"] = np.concatenate([ia[a["edge_i"]], ib[b["edge_i"]]]).astype(np.uint32)
    out["edge_j"] = np.concatenate([ia[a["edge_j"]], ib[b["edge_j"]]]).astype(np.uint32)
    for k in ("rel_aa", "cov6", "inlier_weight"):
        out[k] = np.concatenate([a[k], b[k]])
    out["rot"] = 0.1 * np.random.default_rng(seed + 9).standard_normal((n, 3))
    out["rot"][ia], out["rot"][ib] = a["rot"], b["rot"]
    return out


STEP_LOSSES = {"none": (None, ()), "huber": ("huber", (0.5,)), "tolerant": ("tolerant", (0.05, 0.01))}
STEP_GRAPHS = {"main": step_main_graph, "delta": step_delta_graph, "twocomp": step_two_component_graph}
# every (graph, error type, loss, radius) the device tests linearise at: the CPU test asserts the floor condition on each of them
STEP_CASES = [("main", _abi.ANGLE_AXIS, "huber", 1e4), ("main", _abi.ANGLE_AXIS, "huber", 1e12), ("main", _abi.ANGLE_AXIS, "none", 1e4),
              ("main", _abi.ANGLE_AXIS, "tolerant", 1e4), ("main", _abi.QUATERNION_COSINE, "huber", 1e4),
              ("main", _abi.QUATERNION_NORM, "huber", 1e4), ("main", _abi.ANGLE_AXIS_COVARIANCE, "huber", 1e4),
              ("main", _abi.ANGLE_AXIS_COV_INLIERS, "huber", 1e4), ("twocomp", _abi.ANGLE_AXIS, "huber", 1e4),
              ("delta", _abi.ANGLE_AXIS, "huber", 1e4), ("delta", _abi.ANGLE_AXIS, "huber", 1e12)]
STEP_FLOOR_MAX = 5e-13   # tol / 2 at cg_relative_tolerance = 1e-12: the reference's own floor at the exact solution must stay below
_STEP_CACHE = {}


def step_graph(name):
    if ("g", name) not in _STEP_CACHE:
        _STEP_CACHE[("g", name)] = STEP_GRAPHS[name]()
    return _STEP_CACHE[("g", name)]


def step_reference(name, et, lname, radius):
    """(graph, lin, A, sysm) of a step case, cached per process: the tier-1 edge set per (graph, error type), the corrected
    linearisation per loss, the damped system per radius."""
    g = step_graph(name)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    k1 = ("e", name, et)
    if k1 not in _STEP_CACHE:
        _STEP_CACHE[k1] = edge_set(et, ei, ej, g["rel_aa"], g["rot"], g["cov6"], g["inlier_weight"])
    k2 = ("l", name, et, lname)
    if k2 not in _STEP_CACHE:
        kind, params = STEP_LOSSES[lname]
        lin = corrected(_STEP_CACHE[k1], kind, params)
        if kind == "huber":   # no edge at the knee, where finite differences and a kernel may disagree
            assert np.all(np.abs(lin["s"].astype(float) - 0.25) > 1e-9 * 0.25)
        _STEP_CACHE[k2] = (lin, assemble(lin, n, ei, ej))
    lin, A = _STEP_CACHE[k2]
    k3 = ("s", name, et, lname, radius)
    if k3 not in _STEP_CACHE:
        _STEP_CACHE[k3] = damped_system(A, radius)
    return g, lin, A, _STEP_CACHE[k3]


def step_solution(name, et, lname, radius):
    """delta* = K*^-1 b* (n x 3, long double), cached."""
    k = ("x", name, et, lname, radius)
    if k not in _STEP_CACHE:
        g, lin, A, sysm = step_reference(name, et, lname, radius)
        K = system_matrix(lin, sysm, g["n_cams"], g["edge_i"], g["edge_j"])
        _STEP_CACHE[k] = solve_refined(K, sysm["b"]).reshape(-1, 3)
    return _STEP_CACHE[k]
