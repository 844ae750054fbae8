"""Reference of the bundle adjustment of camera positions and points (include/gsfm_ba.h); a test helper, not a conftest.

Two tiers over one text:
  fp64   numpy float64 throughout: residual, Jacobian, Corrector, assembly, the FULL damped system solved directly (np.linalg.solve),
         the gauge projection and the LM loop.
  hp     the per-observation residual and Jacobian in mpmath (40 digits, the exact Rodrigues rotation of the input doubles), carried in
         numpy long double from there (the construction of position_hp_reference.py): Corrector, assembly, the reduced system Sc and its
         right-hand side, the refined solution (long-double Cholesky plus one refinement step), back-substitution, the LM loop, and the
         rounding floor of the PCG residual.
The tests bound the device by the fp64 tier's own deviation from the hp tier on the same quantity (see `MARGIN`).
"""
import contextlib

import mpmath
import numpy as np

from globalsfmpy_amd import synth

import position_hp_reference as PH

LD = np.longdouble
U = 2.0 ** -53
MP_DPS = 40
# The device and the fp64 tier evaluate the same formulas in the same precision and differ in the ORDER of their sums (lane strides and
# butterflies against numpy's pairwise sums) and in fused multiply-adds.  Either is a few roundings per term away from the exact value,
# so the device's deviation from the hp tier is bounded by a modest multiple of the fp64 tier's; 64 is the constant the existing
# high-precision tests allow per entry (C0 of test_gpu_positions_hp.py, test_gpu_hp_linearization.py).
MARGIN = 64.0

TERM_NAMES = ("FUNCTION_TOLERANCE", "GRADIENT_TOLERANCE", "PARAMETER_TOLERANCE", "NO_CONVERGENCE", "FAILURE")
DEFAULTS = dict(max_num_iterations=100, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e12, min_trust_region_radius=1e-32, min_relative_decrease=1e-3,
                min_lm_diagonal=1e-6, max_lm_diagonal=1e32, remove_gauge=1)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _finish(sc, cam_est, pt_est):
    sc = dict(sc)
    N, T = sc["rot_aa"].shape[0], len(sc["track_ptr"]) - 1
    sc["cam_est"] = np.ones(N, np.uint8) if cam_est is None else np.asarray(cam_est, np.uint8)
    sc["pt_est"] = np.ones(T, np.uint8) if pt_est is None else np.asarray(pt_est, np.uint8)
    tp = sc["track_ptr"].astype(np.int64)
    sc["track_of"] = np.repeat(np.arange(T), np.diff(tp))
    sc["used"] = (sc["cam_est"][sc["obs_cam"]] != 0) & (sc["pt_est"][sc["track_of"]] != 0)
    sc["cam_active"] = np.zeros(N, bool)
    sc["cam_active"][sc["obs_cam"][sc["used"]]] = True
    sc["pt_active"] = np.zeros(T, bool)
    sc["pt_active"][sc["track_of"][sc["used"]]] = True
    return sc


def scene_a(noise_px=0.5, outlier_frac=0.03):
    """12 cameras / 60 tracks, the generator call of test_gpu_triangulation_host.py, one unestimated camera and a few unestimated tracks."""
    s = synth.make_tracks(12, 60, 21, lengths=(2, 3, 4, 5, 8, 12), noise_px=noise_px, outlier_frac=outlier_frac)
    cam_est = np.ones(12, np.uint8)
    cam_est[5] = 0
    pt_est = np.ones(60, np.uint8)
    pt_est[[3, 17, 40]] = 0
    return _finish({k: s[k] for k in ("rot_aa", "cam_pos", "intrinsics", "track_ptr", "obs_cam", "obs_xy", "gt_points")}, cam_est, pt_est)


def scene_b(noise_px=0.5, seed=5):
    """70 cameras: tracks of 2, 8, 9, 64, 65 and 70 observations (both lane-class boundaries) and cameras whose rows hold 3, 63, 64, 65 and
    about 300 observations (the 64-lane row stride): cameras 4, 1, 2, 3 and 0.  Every camera has at least 3 observations."""
    base = synth.make_tracks(70, 1, 33, lengths=(2,), noise_px=0.0)
    rng = np.random.default_rng(seed)
    tracks = [list(range(70)), [0] + list(range(5, 69)), [0] + list(range(5, 68)), list(range(10, 19)), list(range(20, 28)), [30, 45]]
    fill = lambda k: 10 + (7 * k) % 60
    tracks += [[0, 4, 10], [0, 4, 11]]
    for cam, more in ((1, 62), (2, 63), (3, 64)):
        tracks += [[0, cam, fill(k + cam)] for k in range(more)]
    tracks += [[0, fill(k), fill(k + 23)] for k in range(106)]
    T = len(tracks)
    gt = rng.uniform(-2.0, 2.0, (T, 3))
    obs_cam = np.concatenate(tracks).astype(np.uint32)
    track_ptr = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint64)
    track_of = np.repeat(np.arange(T), [len(t) for t in tracks])
    R = synth.aa_to_matrix(base["rot_aa"])
    p = np.einsum("eij,ej->ei", R[obs_cam], gt[track_of] - base["cam_pos"][obs_cam])
    K = base["intrinsics"]
    xy = K[obs_cam, :1] * p[:, :2] / p[:, 2:] + K[obs_cam, 1:] + noise_px * rng.standard_normal((len(obs_cam), 2))
    sc = _finish({"rot_aa": base["rot_aa"], "cam_pos": base["cam_pos"], "intrinsics": K, "track_ptr": track_ptr, "obs_cam": obs_cam, "obs_xy": xy,
                  "gt_points": gt}, None, None)
    rows = np.bincount(obs_cam, minlength=70)
    assert [rows[c] for c in (4, 1, 2, 3)] == [3, 63, 64, 65] and 280 <= rows[0] <= 320, rows[:5]
    assert rows.min() >= 3
    assert sorted(set(np.diff(track_ptr.astype(np.int64)))) == [2, 3, 8, 9, 64, 65, 70]
    return sc


T_CAMERA, T_TRACK = 4, 5   # scene t: the camera (3 rows) and the two-view track [30, 45] whose observations all lie beyond a Tukey cut of 10 px
T_SINGLE = ((0, 7), (0, 40), (1, 0), (1, 33), (2, 17), (3, 4), (4, 2))   # (track, place in the track) of the single displaced observations
T_AT_CUT = ((0, 20, 9.95), (1, 50, 10.05))   # (track, place, |r| at the near start): within 1 % of the cut, one on either side


def scene_t(r=None, shift_px=50.0):
    """Scene b's graph with observations that a Tukey loss of width 10 cuts at the near start (perturbation 0.05, seed 1): every observation
    of camera T_CAMERA, both of track T_TRACK and the T_SINGLE ones in long tracks are displaced by shift_px ALONG their residual at that
    start (so that the residual grows by that much whatever it was), and the T_AT_CUT ones are placed so that their residual there has the
    given norm.  r: scene b's residuals (E x 2) at the start meant, default this module's near start (ba6_reference.py passes its own)."""
    b = scene_b()
    if r is None:
        r = observe_np(b, *perturbed_start(b, 0.05, 0.05, 1))[0]
    tp = b["track_ptr"].astype(np.int64)
    es = set(np.flatnonzero(b["obs_cam"] == T_CAMERA)) | set(range(tp[T_TRACK], tp[T_TRACK + 1])) | {int(tp[t] + k) for t, k in T_SINGLE}
    assert not es & {int(tp[t] + k) for t, k, _ in T_AT_CUT}
    xy = b["obs_xy"].copy()
    unit = r / np.sqrt((r * r).sum(1))[:, None]
    for e in sorted(es):
        xy[e] -= shift_px * unit[e]            # r = projection - xy
    for t, k, norm in T_AT_CUT:
        e = tp[t] + k
        xy[e] += r[e] - norm * unit[e]
    sc = dict(b)
    sc["obs_xy"] = xy
    return sc


def perturbed_start(sc, sigma_cam, sigma_pt, seed):
    rng = np.random.default_rng(seed)
    return sc["cam_pos"] + sigma_cam * rng.standard_normal(sc["cam_pos"].shape), sc["gt_points"] + sigma_pt * rng.standard_normal(sc["gt_points"].shape)


def normalise(sc, cam, pts):
    """active cameras and points with translation and scale removed: (x - mean) / rms, cameras first"""
    x = np.concatenate([np.asarray(cam, float)[sc["cam_active"]], np.asarray(pts, float)[sc["pt_active"]]])
    x = x - x.mean(0)
    return x / np.sqrt((x * x).sum() / len(x))


# ---- per-observation residual and Jacobian --------------------------------------------------------------------------------------
def observe_np(sc, cam, pts):
    """(r: E x 2, J: E x 2 x 3) in float64 for every observation (rows of unused observations are zero)"""
    c, t = sc["obs_cam"], sc["track_of"]
    R = synth.aa_to_matrix(sc["rot_aa"])[c]
    K = sc["intrinsics"][c]
    with np.errstate(all="ignore"):
        p = np.einsum("eij,ej->ei", R, np.asarray(pts, float)[t] - np.asarray(cam, float)[c])
        r = K[:, :1] * p[:, :2] / p[:, 2:] + K[:, 1:] - sc["obs_xy"]
        A = np.zeros((len(c), 2, 3))
        A[:, 0, 0] = A[:, 1, 1] = 1.0
        A[:, 0, 2], A[:, 1, 2] = -p[:, 0] / p[:, 2], -p[:, 1] / p[:, 2]
        J = (K[:, 0] / p[:, 2])[:, None, None] * (A @ R)
    r[~sc["used"]] = 0
    J[~sc["used"]] = 0
    return r, J


def _mp(x):
    return mpmath.mpf(float(x))


def rotation_mp(aa):
    """the exact rotation matrix of the angle-axis doubles (Rodrigues in mpmath), 3 x 3 list"""
    w = [_mp(x) for x in aa]
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    I = [[mpmath.mpf(int(i == j)) for j in range(3)] for i in range(3)]
    if th2 == 0:
        return I
    th = mpmath.sqrt(th2)
    k = [x / th for x in w]
    ct, st = mpmath.cos(th), mpmath.sin(th)
    Kx = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    return [[ct * I[i][j] + st * Kx[i][j] + (1 - ct) * k[i] * k[j] for j in range(3)] for i in range(3)]


def residual_mp(R, K, xy, X, o):
    """(r (2), p (3)) in mpmath"""
    v = [X[j] - o[j] for j in range(3)]
    p = [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]
    return [K[0] * p[0] / p[2] + K[1] - xy[0], K[0] * p[1] / p[2] + K[2] - xy[1]], p


def jacobian_mp(R, K, p):
    fz = K[0] / p[2]
    a = [-p[0] / p[2], -p[1] / p[2]]
    return [[fz * (R[i][j] + a[i] * R[2][j]) for j in range(3)] for i in range(2)]


def _ld(x):
    return LD(mpmath.nstr(x, 25))


_ROT_CACHE = {}


def observe_hp(sc, cam, pts):
    """observe_np's arrays in long double, every used observation evaluated in mpmath from the input doubles"""
    E = len(sc["obs_cam"])
    r, J = np.zeros((E, 2), LD), np.zeros((E, 2, 3), LD)
    with mpmath.workdps(MP_DPS):
        key = sc["rot_aa"].tobytes()
        if key not in _ROT_CACHE:
            _ROT_CACHE[key] = [rotation_mp(a) for a in sc["rot_aa"]]
        Rs = _ROT_CACHE[key]
        camm = [[_mp(x) for x in row] for row in np.asarray(cam, float)]
        ptm = [[_mp(x) for x in row] for row in np.asarray(pts, float)]
        Km = [[_mp(x) for x in row] for row in sc["intrinsics"]]
        for e in np.flatnonzero(sc["used"]):
            c, t = int(sc["obs_cam"][e]), int(sc["track_of"][e])
            re, p = residual_mp(Rs[c], Km[c], [_mp(x) for x in sc["obs_xy"][e]], ptm[t], camm[c])
            Je = jacobian_mp(Rs[c], Km[c], p)
            r[e] = [_ld(x) for x in re]
            J[e] = [[_ld(x) for x in row] for row in Je]
    return r, J


# ---- loss, Corrector, assembly (dtype of the inputs) -----------------------------------------------------------------------------
def loss_rho(kind, a, s):
    """(rho, rho', rho'') at s in the dtype of s.  a: the loss's width, or (width, sigma2) for Geman-McClure: the parameters of
    loss_functions.GemanMcClureLoss in its order, sigma2 entering as it stands (tests/test_oracle_golden.py pins that class to the
    reference project's vectors).  Tukey and Geman-McClure are Ceres' formulas as position_hp_reference.loss_rho states them."""
    one = s.dtype.type(1)
    if kind in (None, "trivial"):
        return s, np.ones_like(s), np.zeros_like(s)
    params = tuple(a) if isinstance(a, (tuple, list)) else (a,)
    a = s.dtype.type(params[0])
    b = a * a
    if kind == "tukey":
        inside = s <= b
        v = np.where(inside, one - s / b, 0)
        return np.where(inside, b / 6 * (one - v * v * v), b / 6), np.where(inside, v * v / 2, 0), np.where(inside, -v / b, 0)
    if kind == "geman_mcclure":
        g2 = s.dtype.type(params[1])
        t = s / b + g2
        return b * g2 * s / (2 * (s + b * g2)), g2 * g2 / (2 * t * t), -(g2 * g2) / (b * t * t * t)
    with np.errstate(all="ignore"):
        if kind == "huber":
            rt = np.sqrt(s)
            out = s > b
            r1 = np.where(out, a / rt, one)
            return np.where(out, 2 * a * rt - b, s), r1, np.where(out, -r1 / (2 * s), 0)
        if kind == "softl1":
            sm = one + s / b
            tmp = np.sqrt(sm)
            r1 = one / tmp
            return 2 * b * (tmp - one), r1, -(r1 / b) / (2 * sm)
    raise ValueError(kind)


# One plausible defect each, of the kind a device kernel could carry: the CPU tests put the fp64 tier WITH the defect where the device's output goes
# in the GPU tests' ratio and require it above 1 (the parity tests would notice).
DEFECTS = {"geman_unsquared": ("geman_mcclure", (10.0, 0.5)), "tukey_without_half": ("tukey", 10.0), "tukey_cut_at_a": ("tukey", 10.0)}
_sound_loss_rho = loss_rho


@contextlib.contextmanager
def defect(name):
    """Within the block this module's loss_rho (which linearise, and through it ba6_reference.linearise, calls) carries the named defect."""
    global loss_rho
    kind = DEFECTS[name][0]

    def bad(k, a, s):
        r0, r1, r2 = _sound_loss_rho(k, a, s)
        if k != kind:
            return r0, r1, r2
        if name == "geman_unsquared":        # sigma2 where sigma2^2 belongs
            g2 = s.dtype.type(a[1])
            return r0, r1 / g2, r2 / g2
        if name == "tukey_without_half":     # rho' = v^2
            return r0, 2 * r1, r2
        beyond = s >= s.dtype.type(a)        # the cut at s < a in place of s <= a^2
        return np.where(beyond, s.dtype.type(a) ** 2 / 6, r0), np.where(beyond, 0, r1), np.where(beyond, 0, r2)
    loss_rho = bad
    try:
        yield
    finally:
        loss_rho = _sound_loss_rho


def linearise(r, J, kind=None, a=None):
    """dict(s, rho, H: E x 3 x 3, a: E x 3, cost, rt, Jt) of the corrected point Jacobian J~ and residual r~ (Ceres' Corrector).  Beyond the
    Tukey cut rho' = 0: the masked-out alpha divides by it (hence the errstate), and J~ and r~ are exactly zero."""
    s = (r * r).sum(1)
    rho0, rho1, rho2 = loss_rho(kind, a, s)
    sq = np.sqrt(rho1)
    mask = (s > 0) & (rho2 > 0)
    with np.errstate(all="ignore"):
        alpha = np.where(mask, 1 - np.sqrt(1 + 2 * s * rho2 / rho1), 0)
        asn = np.where(mask, alpha / np.where(mask, s, 1), 0)
    rJ = np.einsum("ei,eij->ej", r, J)
    Jt = sq[:, None, None] * (J - asn[:, None, None] * r[:, :, None] * rJ[:, None, :])
    rt = (sq / (1 - alpha))[:, None] * r
    return {"s": s, "rho": rho0, "H": np.einsum("eki,ekj->eij", Jt, Jt), "a": np.einsum("eki,ek->ei", Jt, rt), "cost": rho0.sum() / 2, "rt": rt,
            "Jt": Jt}


def assemble(sc, lin):
    """B (N x 3 x 3), C (T x 3 x 3), g (nodes x 3: cameras, then points)"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    dt = lin["H"].dtype
    B, Cm, g = np.zeros((N, 3, 3), dt), np.zeros((T, 3, 3), dt), np.zeros((N + T, 3), dt)
    np.add.at(B, sc["obs_cam"], lin["H"])
    np.add.at(Cm, sc["track_of"], lin["H"])
    np.add.at(g, sc["obs_cam"], -lin["a"])
    np.add.at(g, N + sc["track_of"], lin["a"])
    return {"B": B, "C": Cm, "g": g, "cost": lin["cost"]}


def jacobi_scale(asm, jacobi=True):
    d = np.concatenate([np.einsum("kii->ki", asm["B"]), np.einsum("kii->ki", asm["C"])])
    return 1 / (1 + np.sqrt(d)) if jacobi else np.ones_like(d)


def damped(sc, lin, asm, S, radius, o=DEFAULTS):
    """The scaled, damped pieces of one step: D2, b (nodes x 3), Bt (N), Ct (T) with the damping, Cinv, E (per observation, -S_k H_e S_t)."""
    N = len(sc["cam_est"])
    dt = S.dtype.type
    act = np.concatenate([sc["cam_active"], sc["pt_active"]])
    d = np.concatenate([np.einsum("kii->ki", asm["B"]), np.einsum("kii->ki", asm["C"])])
    D2 = np.where(act[:, None], np.minimum(np.maximum(S * S * d, dt(o["min_lm_diagonal"])), dt(o["max_lm_diagonal"])) / dt(radius), 0)
    b = np.where(act[:, None], S * asm["g"], 0)
    eye = np.eye(3, dtype=S.dtype)
    Bt = S[:N, :, None] * asm["B"] * S[:N, None, :] + D2[:N, :, None] * eye
    Ct = S[N:, :, None] * asm["C"] * S[N:, None, :] + D2[N:, :, None] * eye
    Bt[~sc["cam_active"]] = eye
    Ct[~sc["pt_active"]] = eye
    Cinv = np.array([_inv3(m) for m in Ct]) if len(Ct) else Ct
    Cinv[~sc["pt_active"]] = 0
    E = -S[sc["obs_cam"], :, None] * lin["H"] * S[N + sc["track_of"], None, :]
    return add_cholesky(sc, {"act": act, "D2": D2, "b": b, "Bt": Bt, "Ct": Ct, "Cinv": Cinv, "E": E, "S": S})


def _inv3(m):
    c = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                  [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                  [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]], dtype=m.dtype)
    return c / (m[0, 0] * c[0, 0] + m[0, 1] * c[1, 0] + m[0, 2] * c[2, 0])


def _chol3(m):
    L = np.zeros_like(m)
    for j in range(3):
        L[j, j] = np.sqrt(m[j, j] - (L[j, :j] * L[j, :j]).sum())
        for i in range(j + 1, 3):
            L[i, j] = (m[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def c_solve(dm, t, X):
    """C~_t^-1 X (X: 3 or 3 x k; zero for an inactive point).  fp64: the explicit inverse, as before.  hp: through the Cholesky factor of C~_t.  A
    block that lost rank beyond the Tukey cut is held up by the damping alone and its inverse has entries of 1 / D^2, up to 1e16, next to
    entries of order one: ROUNDED to long double that inverse is wrong by 1e-19 x 1e16 in every entry, while E~ C~^-1 E~^T needs the large part
    (along the block's null vector, which E~ annihilates) to cancel.  The triangular solves keep each part to its own size."""
    if "Cchol" not in dm:
        return dm["Cinv"][t] @ X
    L = dm["Cchol"][t]
    if L[0, 0] == 0:
        return np.zeros_like(X)
    y = np.array(X, LD)
    for i in range(3):
        y[i] = (y[i] - sum(L[i, j] * y[j] for j in range(i))) / L[i, i]
    for i in (2, 1, 0):
        y[i] = (y[i] - sum(L[j, i] * y[j] for j in range(i + 1, 3))) / L[i, i]
    return y


def add_cholesky(sc, dm):
    """damped()'s tail for the hp tier: the factors c_solve reads (zero for an inactive point)"""
    if dm["S"].dtype == LD:
        dm["Cchol"] = np.array([_chol3(m) if a else np.zeros((3, 3), LD) for m, a in zip(dm["Ct"], sc["pt_active"])]).reshape(-1, 3, 3)
    return dm


def full_system(sc, dm):
    """K (3 (N + T) square) and its right-hand side; inactive rows and columns the identity, zero right-hand side"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    n = 3 * (N + T)
    K = np.zeros((n, n), dm["S"].dtype)
    for k in range(N):
        K[3 * k:3 * k + 3, 3 * k:3 * k + 3] = dm["Bt"][k]
    for t in range(T):
        K[3 * (N + t):3 * (N + t) + 3, 3 * (N + t):3 * (N + t) + 3] = dm["Ct"][t]
    for e in np.flatnonzero(sc["used"]):
        k, t = int(sc["obs_cam"][e]), N + int(sc["track_of"][e])
        K[3 * k:3 * k + 3, 3 * t:3 * t + 3] += dm["E"][e]
        K[3 * t:3 * t + 3, 3 * k:3 * k + 3] += dm["E"][e].T
    return K, dm["b"].reshape(n).copy()


def schur_system(sc, dm, absolute=False):
    """(Sc: 3N x 3N, rhs: 3N, Mblk: N x 3 x 3 the Schur-Jacobi blocks).  absolute: |B~| + |E~| |C~^-1| |E~^T| and |b_c| + |E~| |C~^-1| |b_p|,
    the magnitudes behind the rounding floor."""
    N = len(sc["cam_est"])
    f = np.abs if absolute else (lambda z: z)
    sgn = 1 if absolute else -1
    Sc = np.zeros((3 * N, 3 * N), dm["S"].dtype)
    Mb = f(dm["Bt"]).copy()
    rhs = f(dm["b"][:N]).reshape(3 * N).copy()
    for k in range(N):
        Sc[3 * k:3 * k + 3, 3 * k:3 * k + 3] = f(dm["Bt"][k])
    tp = sc["track_ptr"].astype(np.int64)
    for t in np.flatnonzero(sc["pt_active"]):
        es = [e for e in range(tp[t], tp[t + 1]) if sc["used"][e]]
        Ci = f(dm["Cinv"][t])
        bp = f(dm["b"][N + t])
        for e in es:
            k = int(sc["obs_cam"][e])
            EC = f(dm["E"][e]) @ Ci if absolute or "Cchol" not in dm else c_solve(dm, t, dm["E"][e].T).T   # (fp64 tier: the product it always formed)
            rhs[3 * k:3 * k + 3] += sgn * (EC @ bp)
            Mb[k] += sgn * (EC @ f(dm["E"][e]).T)
            for e2 in es:
                m = int(sc["obs_cam"][e2])
                Sc[3 * k:3 * k + 3, 3 * m:3 * m + 3] += sgn * (EC @ f(dm["E"][e2]).T)
    return Sc, rhs, Mb


def back_substitute(sc, dm, yc):
    """y_p = C~^-1 (b_p - E~^T y_c), T x 3"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    acc = dm["b"][N:].copy()
    np.add.at(acc, sc["track_of"], -np.einsum("eij,ei->ej", dm["E"], yc.reshape(N, 3)[sc["obs_cam"]]))
    return np.array([c_solve(dm, t, acc[t]) for t in range(T)]).reshape(T, 3)


def solve_step(sc, lin, asm, S, radius, o=DEFAULTS, hp=False):
    """y (nodes x 3) of (S L S + D^2) y = S g: fp64 by the full system solved directly, hp by the reduced system (refined) and
    back-substitution.  Returns (y, dm)."""
    N = len(sc["cam_est"])
    dm = damped(sc, lin, asm, S, radius, o)
    if hp:
        Sc, rhs, _ = schur_system(sc, dm)
        yc = PH.solve_refined(Sc, rhs)
        return np.concatenate([yc.reshape(N, 3), back_substitute(sc, dm, yc)]), dm
    K, b = full_system(sc, dm)
    return np.linalg.solve(K, b).reshape(-1, 3), dm


def quad_form(sc, lin, delta):
    """delta^T L delta = sum_e d^T H_e d, d = delta_t - delta_k"""
    N = len(sc["cam_est"])
    d = delta[N + sc["track_of"]] - delta[sc["obs_cam"]]
    return np.einsum("ei,eij,ej->", d, lin["H"], d)


def project_step(sc, dm, y, x, gauge=True):
    """delta = -S y on the active nodes; with gauge: minus its mean over the active nodes, then minus its component along v = x - mean(x)"""
    act = dm["act"]
    delta = np.where(act[:, None], -dm["S"] * y, 0)
    if gauge and act.any():
        delta = np.where(act[:, None], delta - delta[act].mean(0), 0)
        v = np.where(act[:, None], x - x[act].mean(0), 0)
        vv = (v * v).sum()
        if vv > 0:
            delta = delta - ((delta * v).sum() / vv) * v
    return delta


def gauge_directions(sc, x):
    """the four null directions of J at x (nodes x 3 each): three translations and the scaling about the centroid, on the active nodes"""
    act = np.concatenate([sc["cam_active"], sc["pt_active"]])[:, None]
    out = [np.where(act, np.eye(3)[c][None, :], 0.0) * np.ones_like(x) for c in range(3)]
    out.append(np.where(act, x - x[act[:, 0]].mean(0), 0.0))
    return out


def apply_J(sc, lin, d):
    """J~ d, E x 2: J~_e (d_t - d_k)"""
    N = len(sc["cam_est"])
    return np.einsum("eij,ej->ei", lin["Jt"], d[N + sc["track_of"]] - d[sc["obs_cam"]])


# ---- the LM loop -------------------------------------------------------------------------------------------------------------------
def lm_solve(sc, cam0, pts0, kind=None, a=None, hp=False, **opts):
    """Ceres 1.14's TrustRegionMinimizer + LevenbergMarquardtStrategy as gsfm_ba.h restates them.  Returns dict(cam, points, termination,
    iterations, successful, unsuccessful, initial_cost, final_cost, decisions: every comparison against a threshold as (name, value,
    threshold), trace: per iteration (accepted, cost))."""
    o = dict(DEFAULTS)
    o.update(opts)
    dt = LD if hp else np.float64
    N = len(sc["cam_est"])
    act = np.concatenate([sc["cam_active"], sc["pt_active"]])
    x = np.concatenate([np.asarray(cam0, float), np.asarray(pts0, float)]).astype(dt)
    obs = observe_hp if hp else observe_np

    def lin_at(xx):
        # (the device holds its iterate in fp64: the hp tier evaluates at the fp64 value of its own iterate)
        xf = np.asarray(xx, np.float64)
        r, J = obs(sc, xf[:N], xf[N:])
        lin = linearise(r.astype(dt), J.astype(dt), kind, a)
        return lin, assemble(sc, lin)
    dec, trace = [], []
    out = {"successful": 0, "unsuccessful": 0}

    def finish(term, it, cost):
        xf = np.asarray(x, np.float64)
        cam, pts = np.array(cam0, float), np.array(pts0, float)
        cam[sc["cam_active"]] = xf[:N][sc["cam_active"]]
        pts[sc["pt_active"]] = xf[N:][sc["pt_active"]]
        out.update(cam=cam, points=pts, termination=term, iterations=it, final_cost=float(cost), decisions=dec, trace=trace)
        return out
    if hp:
        x = x.astype(np.float64).astype(dt)
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
        delta = project_step(sc, dm, y, x, bool(o["remove_gauge"]))
        dg, dld = (delta * asm["g"]).sum(), quad_form(sc, lin, delta)
        model = -dg - dld / 2
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


def ratio(dev, fp64, hp):
    """max |dev - hp| / (MARGIN max(max |fp64 - hp|, u max |hp|)): the bound of the GPU tests (at most 1)"""
    hp = np.asarray(hp, LD)
    e_dev = float(np.abs(np.asarray(dev, LD) - hp).max())
    e_ref = float(np.abs(np.asarray(fp64, LD) - hp).max())
    return e_dev / (MARGIN * max(e_ref, U * float(np.abs(hp).max())))


def decision_margin(decisions):
    """the smallest |value / threshold - 1| over the comparisons with a non-zero threshold (the model test: |value| itself must be > 0)"""
    m = np.inf
    for name, v, th in decisions:
        m = min(m, abs(v / th - 1.0) if th != 0 else (np.inf if v != 0 else 0.0))
    return m


# ---- the PCG residual in the preconditioner norm and its rounding floor ------------------------------------------------------------
def _minv_norm(Mb, vec):
    v = vec.reshape(-1, 3)
    return np.sqrt(sum(v[k] @ np.linalg.solve(Mb[k].astype(np.float64), v[k].astype(np.float64)) for k in range(len(v))))


def pcg_residual_and_floor(sc, dm, yc_dev):
    """(sqrt(r.M^-1 r / b.M^-1 b) of the device's y_c against the hp reduced system, the attainable-accuracy floor
    MARGIN u | |Sc| |y| + |rhs| |_M^-1 / |rhs|_M^-1 with the magnitudes of schur_system(absolute=True))"""
    Sc, rhs, Mb = schur_system(sc, dm)
    Sa, ra, _ = schur_system(sc, dm, absolute=True)
    y = np.asarray(yc_dev, LD).reshape(-1)
    res = rhs - Sc @ y
    nb = _minv_norm(Mb, rhs)
    return float(_minv_norm(Mb, res) / nb), float(MARGIN * U * _minv_norm(Mb, Sa @ np.abs(y) + ra) / nb)


# ---- the cases the CPU and the GPU tests share (computed once per process) ---------------------------------------------------------
LOSS = ("huber", 10.0)   # the pipeline's loss
TUKEY, GEMAN = ("tukey", 10.0), ("geman_mcclure", (10.0, 0.5))
CASES = {   # name: (scene, sigma of the start's perturbation, seed[, loss: default LOSS])
    "a_near": ("a", 0.05, 1), "a_far": ("a", 3.0, 4), "b_near": ("b", 0.05, 1), "b_far": ("b", 2.0, 1),
    # Tukey is not convex and the far starts are not the subject: the near start (seed 1 is scene t's own: its observations are placed at it)
    "t_near_tukey": ("t", 0.05, 1, TUKEY), "a_near_tukey": ("a", 0.05, 1, TUKEY), "a_near_geman": ("a", 0.05, 1, GEMAN),
}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scene(name):
    """a, b, t: noisy; a0, b0: noise-free"""
    return cached(("scene", name), {"a": scene_a, "b": scene_b, "t": scene_t, "a0": lambda: scene_a(0.0, 0.0), "b0": lambda: scene_b(0.0)}[name])


def case_loss(name):
    """(kind, a) of the case: the pipeline's loss unless the case names its own"""
    return CASES[name][3] if len(CASES[name]) > 3 else LOSS


def case_start(name):
    sname, sigma, seed = CASES[name][:3]
    return perturbed_start(scene(sname), sigma, sigma, seed)


def case_solve(name, hp):
    """lm_solve of a case with its loss, fp64 or hp tier"""
    def make():
        c0, p0 = case_start(name)
        return lm_solve(scene(CASES[name][0]), c0, p0, *case_loss(name), hp=hp)
    return cached(("solve", name, hp), make)


def point_linearisation(sname, kind, a, hp):
    """(lin, asm) at the near start of the scene (perturbation 0.05, seed 1)"""
    def make():
        sc = scene(sname)
        c0, p0 = perturbed_start(sc, 0.05, 0.05, 1)
        r, J = (observe_hp if hp else observe_np)(sc, c0, p0)
        lin = linearise(r, J, kind, a)
        return lin, assemble(sc, lin)
    return cached(("lin", sname, kind, a, hp), make)
