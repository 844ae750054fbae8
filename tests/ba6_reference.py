"""Reference of the full bundle adjustment -- orientations, positions and points (include/gsfm_ba6.h); a test helper, not a conftest.

The two tiers of ba_reference.py over one text:
  fp64   numpy float64 throughout: residual, the three Jacobians, Corrector, assembly, the FULL damped system solved directly
         (np.linalg.solve), the seven-direction gauge projection and the LM loop.
  hp     per observation the residual, p and the Jacobians, per camera R(w) and J_l(w), in mpmath (40 digits, from the input doubles; J_l by
         its series below |w| = JL_SERIES_BELOW), carried in numpy long double from there: Corrector, assembly, the reduced system Sc and
         its right-hand side, the refined solution, back-substitution, the LM loop and the rounding floor of the PCG residual.
Scenes, the loss, the Corrector's formulas, MARGIN and the LM rules are ba_reference.py's.  Unknowns are nodes x 3 in the device's order:
N angle-axis vectors, N centres, T points.
"""
import mpmath
import numpy as np

from globalsfmpy_amd import synth

import ba_reference as B
import position_hp_reference as PH
from ba_reference import DEFAULTS, LD, MARGIN, MP_DPS, TERM_NAMES, U, cached, decision_margin, loss_rho, ratio  # noqa: F401  (re-exported for the tests)

JL_SERIES_BELOW = 1e-3   # |w| below which the hp tier sums the series of J_l (20 terms: the remainder is below 1e-120)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
C_ANGLES = (0.0, 1e-9, 0.09, 0.11, 3.1)   # |w| of scene c's cameras 0 .. 4: zero, tiny, either side of jl_and_inverse's branch (0.1), near pi


def scene_c(noise_px=0.5, outlier_frac=0.03, seed=11):
    """Scene a's graph and flags with chosen orientations on cameras 0 .. 4 (C_ANGLES about fixed axes); those cameras are moved to look at
    the point cloud from their old distance, and every observation is regenerated for the new cameras."""
    a = B.scene_a(noise_px, outlier_frac)
    rng = np.random.default_rng(seed)
    rot, pos = a["rot_aa"].copy(), a["cam_pos"].copy()
    axes = np.array([[1.0, 0, 0], [0.6, -0.8, 0.0], [0.0, 0.6, 0.8], [-0.48, 0.6, 0.64], [0.36, 0.48, -0.8]])
    for k, th in enumerate(C_ANGLES):
        rot[k] = th * axes[k]
        pos[k] = -synth.aa_to_matrix(rot[k]).T @ np.array([0.0, 0.0, np.linalg.norm(a["cam_pos"][k])])
    assert np.all(rot[0] == 0.0)
    c, t = a["obs_cam"], a["track_of"]
    p = np.einsum("eij,ej->ei", synth.aa_to_matrix(rot)[c], a["gt_points"][t] - pos[c])
    K = a["intrinsics"]
    xy = K[c, :1] * p[:, :2] / p[:, 2:] + K[c, 1:] + noise_px * rng.standard_normal((len(c), 2))
    out = rng.random(len(c)) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, len(c))
    xy[out] += (rng.uniform(50.0, 300.0, len(c))[:, None] * np.c_[np.cos(ang), np.sin(ang)])[out]
    sc = dict(a)
    sc.update(rot_aa=rot, cam_pos=pos, obs_xy=xy)
    return sc


def scene(name):
    """a, b, c, t: noisy; a0, b0, c0: noise-free.  t is ba_reference.scene_t placed at THIS module's near start (the orientations are perturbed too)."""
    if name == "t":
        return cached(("scene6", name), lambda: B.scene_t(observe_np(B.scene("b"), near_start("b"))[0]))
    if name in ("c", "c0"):
        return cached(("scene6", name), (lambda: scene_c()) if name == "c" else (lambda: scene_c(0.0, 0.0)))
    return B.scene(name)


def perturbed_start(sc, sigma, seed, sigma_rot=None):
    """(rot_aa, cam_pos, points) of the scene, perturbed by N(0, sigma^2) on centres and points and N(0, sigma_rot^2) (default sigma / 10, in
    radians) on the angle-axis coordinates"""
    rng = np.random.default_rng(seed)
    sr = 0.1 * sigma if sigma_rot is None else sigma_rot
    cam = sc["cam_pos"] + sigma * rng.standard_normal(sc["cam_pos"].shape)
    pts = sc["gt_points"] + sigma * rng.standard_normal(sc["gt_points"].shape)
    return sc["rot_aa"] + sr * rng.standard_normal(sc["rot_aa"].shape), cam, pts


def nodes(rot, cam, pts):
    return np.concatenate([np.asarray(rot), np.asarray(cam), np.asarray(pts)])


def split(sc, x):
    N = len(sc["cam_est"])
    return x[:N], x[N:2 * N], x[2 * N:]


def active_nodes(sc):
    return np.concatenate([sc["cam_active"], sc["cam_active"], sc["pt_active"]])


# ---- SO(3) ----------------------------------------------------------------------------------------------------------------------
def skew(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1), np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def left_jacobian_np(w):
    """J_l(w) = I + a [w]x + b [w]x^2, a = (1 - cos t) / t^2, b = (t - sin t) / t^3 (series below t^2 = 1e-4), float64, (..., 3, 3)"""
    w = np.asarray(w, np.float64)
    t2 = (w * w).sum(-1)
    small = t2 < 1e-4
    t = np.sqrt(np.where(small, 1.0, t2))
    a = np.where(small, 0.5 - t2 / 24 + t2 * t2 / 720 - t2 ** 3 / 40320, (1 - np.cos(t)) / t ** 2)
    b = np.where(small, 1.0 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880, (t - np.sin(t)) / t ** 3)
    Wx = skew(w)
    return np.eye(3) + a[..., None, None] * Wx + b[..., None, None] * (Wx @ Wx)


def _mp(x):
    return mpmath.mpf(float(x))


def jl_coefficients_mp(t2, series):
    """(a, b) of J_l at t^2 = t2 in mpmath: the series sum_k (-t2)^k / (2k + 2)! and sum_k (-t2)^k / (2k + 3)!, or the closed forms"""
    if series:
        a = mpmath.fsum((-t2) ** k / mpmath.factorial(2 * k + 2) for k in range(20))
        b = mpmath.fsum((-t2) ** k / mpmath.factorial(2 * k + 3) for k in range(20))
        return a, b
    t = mpmath.sqrt(t2)
    return (1 - mpmath.cos(t)) / t2, (t - mpmath.sin(t)) / (t2 * t)


def left_jacobian_mp(aa):
    """J_l of the angle-axis doubles in mpmath, 3 x 3 list"""
    w = [_mp(x) for x in aa]
    t2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    a, b = jl_coefficients_mp(t2, t2 < _mp(JL_SERIES_BELOW) ** 2)
    Wx = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    W2 = [[sum(Wx[i][k] * Wx[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return [[int(i == j) + a * Wx[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]


# ---- per-observation residual and Jacobians -------------------------------------------------------------------------------------
def observe_np(sc, x):
    """(r: E x 2, Jp: E x 2 x 3, Jr: E x 2 x 3) in float64 at the nodes x; rows of unused observations are zero"""
    rot, cam, pts = split(sc, np.asarray(x, float))
    c, t = sc["obs_cam"], sc["track_of"]
    R = synth.aa_to_matrix(rot)[c]
    Jl = left_jacobian_np(rot)[c]
    K = sc["intrinsics"][c]
    with np.errstate(all="ignore"):
        p = np.einsum("eij,ej->ei", R, pts[t] - cam[c])
        r = K[:, :1] * p[:, :2] / p[:, 2:] + K[:, 1:] - sc["obs_xy"]
        A = np.zeros((len(c), 2, 3))
        A[:, 0, 0] = A[:, 1, 1] = 1.0
        A[:, 0, 2], A[:, 1, 2] = -p[:, 0] / p[:, 2], -p[:, 1] / p[:, 2]
        P = (K[:, 0] / p[:, 2])[:, None, None] * A
        Jp = P @ R
        Jr = -P @ skew(p) @ Jl
    for arr in (r, Jp, Jr):
        arr[~sc["used"]] = 0
    return r, Jp, Jr


_ld = B._ld


def observe_hp(sc, x):
    """observe_np's arrays in long double, every used observation evaluated in mpmath from the input doubles"""
    rot, cam, pts = split(sc, np.asarray(x, np.float64))
    E = len(sc["obs_cam"])
    r, Jp, Jr = np.zeros((E, 2), LD), np.zeros((E, 2, 3), LD), np.zeros((E, 2, 3), LD)
    with mpmath.workdps(MP_DPS):
        Rs = [B.rotation_mp(a) for a in rot]
        Jls = [left_jacobian_mp(a) for a in rot]
        camm = [[_mp(v) for v in row] for row in cam]
        ptm = [[_mp(v) for v in row] for row in pts]
        Km = [[_mp(v) for v in row] for row in sc["intrinsics"]]
        for e in np.flatnonzero(sc["used"]):
            c, t = int(sc["obs_cam"][e]), int(sc["track_of"][e])
            re, p = B.residual_mp(Rs[c], Km[c], [_mp(v) for v in sc["obs_xy"][e]], ptm[t], camm[c])
            fz = Km[c][0] / p[2]
            Pm = [[fz, 0, -fz * p[0] / p[2]], [0, fz, -fz * p[1] / p[2]]]
            px = [[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]
            Ppx = [[sum(Pm[i][k] * px[k][j] for k in range(3)) for j in range(3)] for i in range(2)]
            r[e] = [_ld(v) for v in re]
            Jp[e] = [[_ld(sum(Pm[i][k] * Rs[c][k][j] for k in range(3))) for j in range(3)] for i in range(2)]
            Jr[e] = [[_ld(-sum(Ppx[i][k] * Jls[c][k][j] for k in range(3))) for j in range(3)] for i in range(2)]
    return r, Jp, Jr


def residual_hp(sc, x):
    """the plain residual (E x 2, long double) alone: for central differences"""
    return observe_hp(sc, x)[0]


# ---- Corrector, assembly (dtype of the inputs) -----------------------------------------------------------------------------------
def linearise(r, Jp, Jr, kind=None, a=None):
    """dict(s, rho, cost, rt: E x 2, Jp, Jr: the corrected E x 2 x 3 pieces, Jc = [Jr, -Jp]: E x 2 x 6); the Corrector is ba_reference.linearise's"""
    lp = B.linearise(r, Jp, kind, a)
    lr = B.linearise(r, Jr, kind, a)
    return {"s": lp["s"], "rho": lp["rho"], "cost": lp["cost"], "rt": lp["rt"], "Jp": lp["Jt"], "Jr": lr["Jt"], "Jc": np.concatenate([lr["Jt"], -lp["Jt"]], axis=2)}


def assemble(sc, lin):
    """B (N x 6 x 6, w then o), C (T x 3 x 3), g (nodes x 3)"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    dt = lin["Jp"].dtype
    Bm, Cm, g = np.zeros((N, 6, 6), dt), np.zeros((T, 3, 3), dt), np.zeros((2 * N + T, 3), dt)
    c, t = sc["obs_cam"], sc["track_of"]
    np.add.at(Bm, c, np.einsum("eki,ekj->eij", lin["Jc"], lin["Jc"]))
    np.add.at(Cm, t, np.einsum("eki,ekj->eij", lin["Jp"], lin["Jp"]))
    gc = np.einsum("eki,ek->ei", lin["Jc"], lin["rt"])
    np.add.at(g, c, gc[:, :3])
    np.add.at(g, N + c, gc[:, 3:])
    np.add.at(g, 2 * N + t, np.einsum("eki,ek->ei", lin["Jp"], lin["rt"]))
    return {"B": Bm, "C": Cm, "g": g, "cost": lin["cost"]}


def node_diagonal(asm):
    d = np.einsum("kii->ki", asm["B"])
    return np.concatenate([d[:, :3], d[:, 3:], np.einsum("kii->ki", asm["C"])])


def jacobi_scale(asm, jacobi=True):
    d = node_diagonal(asm)
    return 1 / (1 + np.sqrt(d)) if jacobi else np.ones_like(d)


def damped(sc, lin, asm, S, radius, o=DEFAULTS):
    """The scaled, damped pieces of one step: D2, b (nodes x 3), Bt (N x 6 x 6), Ct, Cinv (T x 3 x 3), E (per observation, 6 x 3: S_k Jc^T Jp S_t)"""
    N = len(sc["cam_est"])
    dt = S.dtype.type
    act = active_nodes(sc)
    d = node_diagonal(asm)
    D2 = np.where(act[:, None], np.minimum(np.maximum(S * S * d, dt(o["min_lm_diagonal"])), dt(o["max_lm_diagonal"])) / dt(radius), 0)
    b = np.where(act[:, None], S * asm["g"], 0)
    S6, D6 = np.concatenate([S[:N], S[N:2 * N]], 1), np.concatenate([D2[:N], D2[N:2 * N]], 1)
    Bt = S6[:, :, None] * asm["B"] * S6[:, None, :] + D6[:, :, None] * np.eye(6, dtype=S.dtype)
    Ct = S[2 * N:, :, None] * asm["C"] * S[2 * N:, None, :] + D2[2 * N:, :, None] * np.eye(3, dtype=S.dtype)
    Bt[~sc["cam_active"]] = np.eye(6, dtype=S.dtype)
    Ct[~sc["pt_active"]] = np.eye(3, dtype=S.dtype)
    Cinv = np.array([B._inv3(m) for m in Ct]) if len(Ct) else Ct
    Cinv[~sc["pt_active"]] = 0
    E = S6[sc["obs_cam"], :, None] * np.einsum("eki,ekj->eij", lin["Jc"], lin["Jp"]) * S[2 * N + sc["track_of"], None, :]
    return B.add_cholesky(sc, {"act": act, "D2": D2, "b": b, "Bt": Bt, "Ct": Ct, "Cinv": Cinv, "E": E, "S": S, "b6": np.concatenate([b[:N], b[N:2 * N]], 1)})


def cam_index(N, k):
    """the six places of camera k in the flattened node vector"""
    return np.r_[3 * k:3 * k + 3, 3 * (N + k):3 * (N + k) + 3]


def full_system(sc, dm):
    """K (3 (2N + T) square, node order) and its right-hand side; inactive rows and columns the identity, zero right-hand side"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    n = 3 * (2 * N + T)
    K = np.zeros((n, n), dm["S"].dtype)
    for k in range(N):
        K[np.ix_(cam_index(N, k), cam_index(N, k))] = dm["Bt"][k]
    for t in range(T):
        i = 3 * (2 * N + t)
        K[i:i + 3, i:i + 3] = dm["Ct"][t]
    for e in np.flatnonzero(sc["used"]):
        ik, it = cam_index(N, int(sc["obs_cam"][e])), 3 * (2 * N + int(sc["track_of"][e])) + np.arange(3)
        K[np.ix_(ik, it)] += dm["E"][e]
        K[np.ix_(it, ik)] += dm["E"][e].T
    return K, dm["b"].reshape(n).copy()


def schur_system(sc, dm, absolute=False):
    """(Sc: 6N x 6N, rhs: 6N, Mblk: N x 6 x 6 the Schur-Jacobi blocks), per camera w then o.  absolute: the magnitudes behind the rounding floor."""
    N = len(sc["cam_est"])
    f = np.abs if absolute else (lambda z: z)
    sgn = 1 if absolute else -1
    Sc = np.zeros((6 * N, 6 * N), dm["S"].dtype)
    Mb = f(dm["Bt"]).copy()
    rhs = f(dm["b6"]).reshape(6 * N).copy()
    for k in range(N):
        Sc[6 * k:6 * k + 6, 6 * k:6 * k + 6] = f(dm["Bt"][k])
    tp = sc["track_ptr"].astype(np.int64)
    Sc4, rhs6 = Sc.reshape(N, 6, N, 6).transpose(0, 2, 1, 3), rhs.reshape(N, 6)   # (views: block (k, m) of Sc, row k of rhs)
    for t in np.flatnonzero(sc["pt_active"]):
        es = np.arange(tp[t], tp[t + 1])[sc["used"][tp[t]:tp[t + 1]]]
        ks = sc["obs_cam"][es].astype(np.int64)
        Et = f(dm["E"][es])
        # (ba_reference.c_solve: the hp tier never multiplies by the rounded inverse)
        EC = Et @ f(dm["Cinv"][t]) if absolute or "Cchol" not in dm else B.c_solve(dm, t, np.concatenate(Et, 0).T).T.reshape(Et.shape)
        np.add.at(rhs6, ks, sgn * (EC @ f(dm["b"][2 * N + t])))
        np.add.at(Mb, ks, sgn * np.einsum("aij,akj->aik", EC, Et))
        np.add.at(Sc4, (ks[:, None], ks[None, :]), sgn * np.einsum("aij,bkj->abik", EC, Et))
    return Sc, rhs, Mb


def back_substitute(sc, dm, yc):
    """y_p = C~^-1 (b_p - E~^T y_c), T x 3; yc: 6N (per camera w then o)"""
    N = len(sc["cam_est"])
    acc = dm["b"][2 * N:].copy()
    np.add.at(acc, sc["track_of"], -np.einsum("eij,ei->ej", dm["E"], yc.reshape(N, 6)[sc["obs_cam"]]))
    return np.array([B.c_solve(dm, t, acc[t]) for t in range(len(acc))]).reshape(len(acc), 3)


def cam6_to_nodes(y6):
    y6 = y6.reshape(-1, 6)
    return np.concatenate([y6[:, :3], y6[:, 3:]])


def solve_step(sc, lin, asm, S, radius, o=DEFAULTS, hp=False):
    """y (nodes x 3) of (S L S + D^2) y = S g: fp64 by the full system solved directly, hp by the reduced system (refined) and
    back-substitution.  Returns (y, dm)."""
    dm = damped(sc, lin, asm, S, radius, o)
    if hp:
        Sc, rhs, _ = schur_system(sc, dm)
        yc = PH.solve_refined(Sc, rhs)
        return np.concatenate([cam6_to_nodes(yc), back_substitute(sc, dm, yc)]), dm
    K, b = full_system(sc, dm)
    return np.linalg.solve(K, b).reshape(-1, 3), dm


def apply_J(sc, lin, d):
    """J~ d, E x 2: Jr d_rot + Jp (d_t - d_pos)"""
    N = len(sc["cam_est"])
    c, t = sc["obs_cam"], sc["track_of"]
    return np.einsum("eij,ej->ei", lin["Jr"], d[c]) + np.einsum("eij,ej->ei", lin["Jp"], d[2 * N + t] - d[N + c])


def quad_form(sc, lin, delta):
    jd = apply_J(sc, lin, delta)
    return (jd * jd).sum()


def _inv3_rows(M):
    return np.array([B._inv3(m) for m in M])


def gauge_directions(sc, x, jl=None):
    """the seven null directions of J at x (nodes x 3 each, dtype of x): three translations, the scaling about the centroid of the active
    centres and points, three rotations (phi x X, phi x o, -J_l(w)^-T phi); zero on inactive nodes.  jl: J_l per camera (N x 3 x 3, dtype of x),
    default the float64 closed form."""
    N = len(sc["cam_est"])
    dt = x.dtype
    act = active_nodes(sc)
    pp = act.copy()
    pp[:N] = False
    out = []
    for c in range(3):
        v = np.zeros_like(x)
        v[pp, c] = 1
        out.append(v)
    v = np.zeros_like(x)
    v[pp] = x[pp] - x[pp].mean(0)
    out.append(v)
    Jl = left_jacobian_np(np.asarray(x[:N], np.float64)).astype(dt) if jl is None else jl
    with np.errstate(all="ignore"):
        JiT = np.transpose(_inv3_rows(Jl), (0, 2, 1))
    for c in range(3):
        phi = np.zeros(3, dt)
        phi[c] = 1
        v = np.zeros_like(x)
        v[pp] = np.cross(phi, x[pp])
        v[:N][sc["cam_active"]] = -(JiT @ phi)[sc["cam_active"]]
        out.append(v)
    return out


def jl_hp(sc, x):
    """J_l of the orientations in x, mpmath -> long double (N x 3 x 3)"""
    N = len(sc["cam_est"])
    with mpmath.workdps(MP_DPS):
        return np.array([[[_ld(v) for v in row] for row in left_jacobian_mp(a)] for a in np.asarray(x[:N], np.float64)], LD)


def _solve_small(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, p]], b[[j, p]] = A[[p, j]], b[[p, j]]
        for i in range(j + 1, n):
            f = A[i, j] / A[j, j]
            A[i, j:] -= f * A[j, j:]
            b[i] -= f * b[j]
    y = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        y[i] = (b[i] - A[i, i + 1:] @ y[i + 1:]) / A[i, i]
    return y


def project_step(sc, dm, y, x, gauge=True, jl=None):
    """delta = -S y on the active nodes; with gauge: minus its orthogonal projection onto the span of the seven gauge directions"""
    act = dm["act"]
    delta = np.where(act[:, None], -dm["S"] * y, 0)
    if gauge and act.any():
        V = np.array([v.reshape(-1) for v in gauge_directions(sc, x, jl)])
        c = _solve_small(V @ V.T, V @ delta.reshape(-1))
        delta = delta - (c @ V).reshape(-1, 3)
    return delta


# ---- alignment: a similarity transform removed ------------------------------------------------------------------------------------
def align(sc, rot, cam, pts, ref_cam, ref_pts):
    """The estimate (rot_aa, cam_pos, points) mapped by the similarity (s, Q, t) that brings its active centres and points closest (least
    squares, Umeyama) to the reference's, after the reference itself is normalised to zero mean and unit rms.  Returns one array: the
    active cameras' rotation matrices R Q^T (9 each), then the mapped active centres and points (3 each), flattened."""
    ca, pa = sc["cam_active"], sc["pt_active"]
    Y = np.concatenate([np.asarray(ref_cam, float)[ca], np.asarray(ref_pts, float)[pa]])
    Y = Y - Y.mean(0)
    Y = Y / np.sqrt((Y * Y).sum() / len(Y))
    X = np.concatenate([np.asarray(cam, float)[ca], np.asarray(pts, float)[pa]])
    mx = X.mean(0)
    Xc = X - mx
    Um, sv, Vt = np.linalg.svd(Y.T @ Xc)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Um @ Vt))])
    Q = Um @ D @ Vt
    s = (sv * np.diag(D)).sum() / (Xc * Xc).sum()
    Xa = s * Xc @ Q.T
    Rm = synth.aa_to_matrix(np.asarray(rot, float)[ca]) @ Q.T
    return np.concatenate([Rm.reshape(-1), Xa.reshape(-1)])


# ---- the LM loop (the rules of ba_reference.lm_solve) ------------------------------------------------------------------------------
def lm_solve(sc, x0, kind=None, a=None, hp=False, **opts):
    """Ceres 1.14's TrustRegionMinimizer + LevenbergMarquardtStrategy as gsfm_ba6.h restates them, from the nodes x0.  Returns dict(x, rot, cam,
    points, termination, iterations, successful, unsuccessful, initial_cost, final_cost, decisions, trace) as ba_reference.lm_solve."""
    o = dict(DEFAULTS)
    o.update(opts)
    dt = LD if hp else np.float64
    act = active_nodes(sc)
    x0 = np.asarray(x0, np.float64)
    x = x0.astype(dt)
    obs = observe_hp if hp else observe_np

    def lin_at(xx):
        # (the device holds its iterate in fp64: the hp tier evaluates at the fp64 value of its own iterate)
        r, Jp, Jr = obs(sc, np.asarray(xx, np.float64))
        lin = linearise(r.astype(dt), Jp.astype(dt), Jr.astype(dt), kind, a)
        return lin, assemble(sc, lin)
    dec, trace = [], []
    out = {"successful": 0, "unsuccessful": 0}

    def finish(term, it, cost):
        xf = x0.copy()
        xf[act] = np.asarray(x, np.float64)[act]
        rot, cam, pts = split(sc, xf)
        out.update(x=xf, rot=rot, cam=cam, points=pts, termination=term, iterations=it, final_cost=float(cost), decisions=dec, trace=trace)
        return out
    lin, asm = lin_at(x)
    S = jacobi_scale(asm)
    cost = lin["cost"]
    out["initial_cost"] = float(cost)
    gmax = np.abs(asm["g"][act]).max() if act.any() else dt(0)
    dec.append(("gradient", float(gmax), o["gradient_tolerance"]))
    if gmax <= o["gradient_tolerance"]:
        return finish(1, 0, cost)
    radius, dfac, invalid, it, last_ok = dt(o["initial_trust_region_radius"]), dt(2), 0, 0, False
    while True:
        if it >= o["max_num_iterations"]:
            return finish(3, it, cost)
        if last_ok:
            dec.append(("gradient", float(gmax), o["gradient_tolerance"]))
            if gmax <= o["gradient_tolerance"]:
                return finish(1, it, cost)
        if radius <= o["min_trust_region_radius"]:
            return finish(4, it, cost)
        it += 1
        last_ok = False
        y, dm = solve_step(sc, lin, asm, S, radius, o, hp)
        delta = project_step(sc, dm, y, x, bool(o["remove_gauge"]), jl_hp(sc, x) if hp else None)
        dg, jd2 = (delta * asm["g"]).sum(), quad_form(sc, lin, delta)
        model = -dg - jd2 / 2
        dec.append(("model", float(model), 0.0))
        if not (np.isfinite(model) and model > 0):
            invalid += 1
            if invalid >= 5:
                return finish(4, it, cost)
            radius, dfac = radius / dfac, dfac * 2
            out["unsuccessful"] += 1
            trace.append((False, float(cost)))
            continue
        invalid = 0
        cand = (x + delta).astype(np.float64).astype(dt)
        clin, casm = lin_at(cand)
        ccost = clin["cost"]
        if not np.isfinite(ccost):
            ccost = dt(np.finfo(np.float64).max)
        step_norm, x_norm = np.sqrt((delta * delta).sum()), np.sqrt((x[act] * x[act]).sum())
        change = cost - ccost
        dec.append(("parameter", float(step_norm), float(o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]))))
        if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            return finish(2, it, cost)
        dec.append(("function", float(abs(change)), float(o["function_tolerance"] * cost)))
        if abs(change) <= o["function_tolerance"] * cost:
            return finish(0, it, cost)
        rel = change / model
        dec.append(("relative_decrease", float(rel), o["min_relative_decrease"]))
        if rel > o["min_relative_decrease"]:
            x, cost, lin, asm = cand, ccost, clin, casm
            gmax = np.abs(asm["g"][act]).max()
            radius = min(dt(o["max_trust_region_radius"]), radius / max(dt(1) / 3, 1 - (2 * rel - 1) ** 3))
            dfac = dt(2)
            out["successful"] += 1
            last_ok = True
        else:
            radius, dfac = radius / dfac, dfac * 2
            out["unsuccessful"] += 1
        trace.append((last_ok, float(cost)))


# ---- the PCG residual in the preconditioner norm and its rounding floor ------------------------------------------------------------
def _minv_norm(Mb, vec):
    v = vec.reshape(-1, 6)
    return np.sqrt(sum(v[k] @ np.linalg.solve(Mb[k].astype(np.float64), v[k].astype(np.float64)) for k in range(len(v))))


def pcg_residual_and_floor(sc, dm, yc_dev):
    """ba_reference.pcg_residual_and_floor for the 6 x 6-block reduced system; yc_dev: N x 6"""
    Sc, rhs, Mb = schur_system(sc, dm)
    Sa, ra, _ = schur_system(sc, dm, absolute=True)
    y = np.asarray(yc_dev, LD).reshape(-1)
    res = rhs - Sc @ y
    nb = _minv_norm(Mb, rhs)
    return float(_minv_norm(Mb, res) / nb), float(MARGIN * U * _minv_norm(Mb, Sa @ np.abs(y) + ra) / nb)


# ---- the cases the CPU and the GPU tests share (computed once per process) ---------------------------------------------------------
LOSS = B.LOSS
NEAR = (0.05, 1)   # sigma and seed of the start of the linearisation and step tests
CASES = {   # name: (scene, sigma of the start's perturbation, seed); chosen on the CPU: tests/test_ba6_reference.py asserts the conditions
    "a_near": ("a", 0.05, 1), "a_far": ("a", 3.0, 1), "b_near": ("b", 0.05, 1), "b_far": ("b", 2.0, 5), "c_near": ("c", 0.05, 1), "c_far": ("c", 3.0, 16),
    # a fourth entry is the case's loss (default LOSS); the near start, as in ba_reference.CASES (scene t's observations are placed at NEAR)
    "t_near_tukey": ("t", 0.05, 1, B.TUKEY), "a_near_tukey": ("a", 0.05, 1, B.TUKEY), "a_near_geman": ("a", 0.05, 1, B.GEMAN),
}


def near_start(sname):
    return nodes(*perturbed_start(scene(sname), *NEAR))


def case_loss(name):
    return CASES[name][3] if len(CASES[name]) > 3 else LOSS


def case_start(name):
    sname, sigma, seed = CASES[name][:3]
    return nodes(*perturbed_start(scene(sname), sigma, seed))


def case_solve(name, hp):
    return cached(("solve6", name, hp), lambda: lm_solve(scene(CASES[name][0]), case_start(name), *case_loss(name), hp=hp))


def point_observation(sname, hp):
    return cached(("obs6", sname, hp), lambda: (observe_hp if hp else observe_np)(scene(sname), near_start(sname)))


def point_linearisation(sname, kind, a, hp):
    """(lin, asm) at the near start of the scene"""
    def make():
        lin = linearise(*point_observation(sname, hp), kind, a)
        return lin, assemble(scene(sname), lin)
    return cached(("lin6", sname, kind, a, hp), make)
