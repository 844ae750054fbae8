"""High-precision reference of the position residual, its linearisation and one LM step (test helper, not a conftest).

Tier 1 (mpmath, 50 digits, per edge): the world direction d = R(aa_i)^T t_ij from the exact input doubles with the exact rotation (not
Ceres' first-order form below theta^2 = DBL_EPSILON: that branch's truncation error, theta^2 / 2 |t| <= u |t| at its switch, is the
reference's own and lies inside the bounds), the residual r = w / n - d with w = c_j - c_i and the guard n := 1 below 1e-12 decided on
the exact n, and the Jacobian dr/dc_j by central differences (h small against n), so that nothing relies on the closed form
(I - u u^T) / n.  dr/dc_i = -dr/dc_j.

Tier 2 (numpy longdouble): the per-edge dicts of hp_reference (r, Ji = -P, Jj = +P, e_mag, Jw_*), so that hp_reference.corrected,
assemble, matvec and normal_matrix apply unchanged, and the damped step system of one LM step: S, D^2 with its clamps, K = S L S + D^2,
b = S g, inactive rows the identity with a zero right-hand side, y by a long-double Cholesky plus one refinement step, delta = -S y with
the scale gauge projected out, and the model cost change -delta.g - delta^T L delta / 2.

Error scales (in units of u, multiplied by c u in the tests).  The device forms w = c_m - c_k by one correctly rounded subtraction of the
exact inputs, so w carries a relative error u per component however much it cancels; n, u = w / n and r = u - d then add a few
roundings of size u (1 + |d|), and d's rotation a few of size u |t|:  e_mag = 1 + |t| per component.  The Jacobian (I - u u^T) / n is
formed from u and n with a few roundings of size u / n per entry (1 - u_k^2 may cancel to nothing, its error does not): Jw = 2 / n per
column, 0 in the guard branch, whose Jacobian is the exact identity.
"""
import mpmath
import numpy as np

import hp_reference as H

MP_DPS = 50   # (w = c_j - c_i of inputs near 1e8 keeps ~40 digits of an n near 1e-11: the differences below need them)
U = H.U
LD = H.LD
NORM_TOL = 1e-12   # Theia's kNormTolerance
_HP_LOSS_RHO = H.loss_rho


def _mp(x):
    return mpmath.mpf(float(x))


def direction(aa, t):
    """d = R(aa)^T t with the exact rotation (Rodrigues in mpmath) of the exact input doubles; mpmath list of 3."""
    w = [_mp(x) for x in aa]
    tv = [_mp(x) for x in t]
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if th2 == 0:
        return tv
    th = mpmath.sqrt(th2)
    k = [x / th for x in w]
    ct, st = mpmath.cos(th), mpmath.sin(th)
    kt = k[0] * tv[0] + k[1] * tv[1] + k[2] * tv[2]
    cross = [k[1] * tv[2] - k[2] * tv[1], k[2] * tv[0] - k[0] * tv[2], k[0] * tv[1] - k[1] * tv[0]]
    # R^T t = rotation by -theta: t cos - (k x t) sin + k (k.t) (1 - cos)
    return [tv[c] * ct - cross[c] * st + k[c] * kt * (1 - ct) for c in range(3)]


def residual(ci, cj, d):
    """(r, n, unit) in mpmath: r = w / n - d, n = |w| (n := 1 below 1e-12, decided on the exact n), unit: n was kept."""
    w = [cj[k] - ci[k] for k in range(3)]
    n = mpmath.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    unit = not (n < NORM_TOL)
    if not unit:
        n = mpmath.mpf(1)
    return [w[k] / n - d[k] for k in range(3)], n, unit


def edge_linearise(ci, cj, d):
    """(r, J, n, unit): J = dr/dc_j (3 x 3 mpmath) by central differences.  h = 1e-12 n where n is kept (truncation (h / n)^2, cancellation
    10^-50 |c| / h, both far below u); in the guard branch r is linear in c_j and h = 1e-3 (1e-12 - n) keeps the perturbed points inside it."""
    ci, cj = [_mp(x) for x in ci], [_mp(x) for x in cj]
    r, n, unit = residual(ci, cj, d)
    nn = mpmath.sqrt(sum((cj[k] - ci[k]) ** 2 for k in range(3)))
    h = mpmath.mpf("1e-12") * nn if unit else mpmath.mpf("1e-3") * (mpmath.mpf(NORM_TOL) - nn)
    J = [[None] * 3 for _ in range(3)]
    for c in range(3):
        cp, cm = list(cj), list(cj)
        cp[c] += h
        cm[c] -= h
        rp, rm = residual(ci, cp, d)[0], residual(ci, cm, d)[0]
        for k in range(3):
            J[k][c] = (rp[k] - rm[k]) / (2 * h)
    return r, J, n, unit


def _ld(x):
    return LD(mpmath.nstr(x, 25))


def edge_set(edge_i, edge_j, rel_t, rot_aa, pos):
    """Tier 1 for every edge, as long-double arrays in hp_reference's per-edge layout: r (E x 3), Ji = -P, Jj = +P (E x 3 x 3), the
    error scales e_mag (E x 3) and Jw_i, Jw_j (E x 3), and d (E x 3), n (E), unit (E) for the tests."""
    E = len(edge_i)
    out = {"r": np.zeros((E, 3), LD), "Ji": np.zeros((E, 3, 3), LD), "Jj": np.zeros((E, 3, 3), LD), "e_mag": np.zeros((E, 3), LD),
           "Jw_i": np.zeros((E, 3), LD), "Jw_j": np.zeros((E, 3), LD), "d": np.zeros((E, 3), LD), "n": np.zeros(E, LD),
           "unit": np.zeros(E, bool)}
    with mpmath.workdps(MP_DPS):
        for e in range(E):
            i, j = int(edge_i[e]), int(edge_j[e])
            d = direction(rot_aa[i], rel_t[e])
            r, J, n, unit = edge_linearise(pos[i], pos[j], d)
            out["r"][e] = [_ld(x) for x in r]
            P = np.array([[_ld(x) for x in row] for row in J], dtype=LD)
            out["Jj"][e], out["Ji"][e] = P, -P
            out["d"][e] = [_ld(x) for x in d]
            out["n"][e], out["unit"][e] = _ld(n), unit
            out["e_mag"][e] = 1.0 + float(np.linalg.norm(np.asarray(rel_t[e], float)))
            if unit:
                out["Jw_i"][e] = out["Jw_j"][e] = 2.0 / float(n)
    return out


# ---- losses the device has as LM_SIMPLE leaves beyond hp_reference's ----
def loss_rho(kind, params, s):
    """hp_reference.loss_rho plus Tukey and Geman-McClure (Ceres' formulas in long double)."""
    s = np.asarray(s, LD)
    one = LD(1)
    if kind == "tukey":
        a2 = LD(params[0]) ** 2
        inside = s <= a2
        v = np.where(inside, one - s / a2, 0)
        return (np.where(inside, a2 / 6 * (one - v ** 3), a2 / 6), np.where(inside, v * v / 2, 0), np.where(inside, -v / a2, 0),
                np.where(inside, a2 / 6 * (one + v ** 3), a2 / 6))
    if kind == "geman_mcclure":
        a2, g2 = LD(params[0]) ** 2, LD(params[1])
        t = s / a2 + g2
        return (a2 * g2 * s / (2 * (s + a2 * g2)), g2 * g2 / (2 * t * t), -(g2 * g2) / (a2 * t ** 3), a2 * g2 * s / (2 * (s + a2 * g2)))
    if kind == "scaled":
        r0, r1, r2, sc = loss_rho(params[0][0], params[0][1], s)
        k = LD(params[1])
        return k * r0, k * r1, k * r2, k * sc
    return _HP_LOSS_RHO(kind, params, s)


def corrected(ref, kind=None, params=()):
    """hp_reference.corrected with this module's losses (Tukey and Geman-McClure included)."""
    saved = H.loss_rho
    H.loss_rho = loss_rho
    try:
        with np.errstate(divide="ignore", invalid="ignore"):   # (rho' = 0 beyond the Tukey cut: the Corrector's masked-out alpha)
            return H.corrected(ref, kind, params)
    finally:
        H.loss_rho = saved


# ---- one LM step in long double ----
def step_system(lin, n_cams, edge_i, edge_j, active, radius, min_diag=1e-6, max_diag=1e32, jacobi=True):
    """The damped, scaled system of one LM step: dict of L (3N x 3N), g (3N), S (3N), D2 (3N), K, b, with inactive rows and columns
    the identity and zero right-hand side, as the device sets them up."""
    A = H.assemble(lin, n_cams, edge_i, edge_j)
    L = H.normal_matrix(lin, n_cams, edge_i, edge_j)
    n = 3 * n_cams
    g = A["g"].reshape(n)
    dg = np.diagonal(L).copy()
    S = (1 / (1 + np.sqrt(dg))) if jacobi else np.ones(n, LD)
    act = np.repeat(np.asarray(active, bool), 3)
    D2 = np.minimum(np.maximum(S * S * dg, LD(min_diag)), LD(max_diag)) / LD(radius)
    K = S[:, None] * L * S[None, :] + np.diag(D2)
    off = np.flatnonzero(~act)
    K[off, :] = 0
    K[:, off] = 0
    K[off, off] = 1
    D2 = np.where(act, D2, 0)
    b = np.where(act, S * g, 0)
    return {"A": A, "L": L, "g": g, "S": S, "D2": D2, "K": K, "b": b, "act": act, "diagL": dg}


def cholesky_factor(K):
    """Lower Cholesky factor of a symmetric positive definite K in long double."""
    L = np.array(K, LD)
    n = L.shape[0]
    for k in range(n):
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return np.tril(L)


def cholesky_apply(L, b):
    x = np.array(b, LD)
    n = len(x)
    for k in range(n):
        x[k] /= L[k, k]
        x[k + 1:] -= L[k + 1:, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] /= L[k, k]
        x[:k] -= L[k, :k] * x[k]
    return x


def solve_refined(K, b):
    """y with K y = b: long-double Cholesky (hp_reference.cholesky_solve's algorithm, factored once) plus one step of refinement."""
    L = cholesky_factor(K)
    y = cholesky_apply(L, b)
    return y + cholesky_apply(L, b - K @ y)


def project_step(y, sys, pos, fixed, gauge=True):
    """delta = -S y on active rows, its component along v = x - x_fixed (active rows) removed; the model cost change."""
    act = sys["act"]
    delta = np.where(act, -sys["S"] * y, 0)
    x = np.asarray(pos, LD).reshape(-1)
    v = np.zeros_like(delta)
    if gauge and fixed >= 0:
        v = np.where(act, x - np.tile(x[3 * fixed:3 * fixed + 3], len(x) // 3), 0)
    vv = v @ v
    if vv > 0:
        delta = delta - (delta @ v / vv) * v
    dg = delta @ sys["g"]
    dld = delta @ (sys["L"] @ delta)
    return delta, v, -dg - dld / 2, dg, dld
