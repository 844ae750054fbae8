"""Reference of the full bundle adjustment with free focal lengths (include/gsfm_ba7.h); a test helper, not a conftest.

The two tiers of ba6_reference.py (numpy float64; mpmath 40 digits, then long double) extended by the focal coordinate.  What does not know
the node layout is ba6_reference.py's and ba_reference.py's own (the observation of the six-coordinate problem, the Corrector, the points'
Cholesky solves, the refined solve, the gauge directions, the alignment); the LM loop, the gauge projection, the quadratic form, the Jacobi
scale and the PCG floor are ba6_reference.py's TEXT run over this module's layout (_over_this_layout); what is written here is what the
seventh coordinate changes: the layout, J_f, the 7 x 7 blocks.
Unknowns are nodes x 3 in the device's order: N angle-axis vectors, N centres, N intrinsics nodes (f, 0, 0), T points.  A scene is
ba6_reference's with "focal_free" (N flags); the focal length comes from the nodes, column 0 of sc["intrinsics"] is the generator's.
"""
import types

import mpmath
import numpy as np

import ba_reference as B
import ba6_reference as R6
import position_hp_reference as PH
from ba_reference import DEFAULTS, LD, MARGIN, MP_DPS, TERM_NAMES, U, cached, decision_margin, loss_rho, ratio  # noqa: F401  (re-exported for the tests)
from ba6_reference import _solve_small, align, jl_hp  # noqa: F401

W = 7   # coordinates per camera: w (3), o (3), f


def _over_this_layout(f):
    """f's text with this module's functions in place of ba6_reference's: one text for both layouts.  The rebound functions resolve these
    names HERE (tests/test_ba7_reference.py holds the list against their code objects, so a name that ba6_reference starts to use fails
    there and not silently):
      lm_solve                DEFAULTS LD np active_nodes observe_hp observe_np linearise assemble split jacobi_scale solve_step project_step
                              jl_hp quad_form
      project_step            np gauge_directions _solve_small
      quad_form               apply_J
      jacobi_scale            node_diagonal np
      pcg_residual_and_floor  schur_system np LD _minv_norm MARGIN U"""
    return types.FunctionType(f.__code__, globals(), f.__name__, f.__defaults__, f.__closure__)


# ---- scenes and starts ----------------------------------------------------------------------------------------------------------
NEAR = (0.05, 1, 0.01)   # sigma, seed and relative sigma of the focal lengths of the start of the linearisation and step tests


def scene(name, focal_free=None):
    """ba6_reference's scenes a, b, c, a0, b0, c0; t is ba_reference.scene_t placed at THIS module's near start (the focal lengths are
    perturbed too).  focal_free: N flags, default all free."""
    def make():
        if name == "t":
            sc = B.scene_t(observe_np(scene("b"), near_start("b"))[0])
        else:
            sc = dict(R6.scene(name))
        sc["focal_free"] = np.ones(len(sc["cam_est"]), bool)
        return sc
    sc = cached(("scene7", name), make)
    if focal_free is not None:
        sc = dict(sc)
        sc["focal_free"] = np.asarray(focal_free, bool)
    return sc


def perturbed_start(sc, sigma, seed, sigma_f):
    """(rot_aa, cam_pos, focal, points): ba6_reference.perturbed_start, and the generator's focal lengths times 1 + N(0, sigma_f^2)"""
    rot, cam, pts = R6.perturbed_start(sc, sigma, seed)
    f = sc["intrinsics"][:, 0] * (1 + sigma_f * np.random.default_rng(seed + 7000).standard_normal(len(cam)))
    return rot, cam, f, pts


def nodes(rot, cam, focal, pts):
    f = np.zeros((len(cam), 3))
    f[:, 0] = focal
    return np.concatenate([np.asarray(rot), np.asarray(cam), f, np.asarray(pts)])


def split(sc, x):
    """(rot_aa, cam_pos, points); the focal lengths are focal_of(sc, x)"""
    N = len(sc["cam_est"])
    return x[:N], x[N:2 * N], x[3 * N:]


def focal_of(sc, x):
    N = len(sc["cam_est"])
    return x[2 * N:3 * N, 0]


def active_nodes(sc):
    return np.concatenate([sc["cam_active"], sc["cam_active"], sc["cam_active"] & sc["focal_free"], sc["pt_active"]])


def _six(sc, x):
    """the scene with the focal lengths of x in its intrinsics, and the nodes of ba6_reference's layout"""
    N = len(sc["cam_est"])
    s6 = dict(sc)
    s6["intrinsics"] = np.array(sc["intrinsics"], np.float64)
    s6["intrinsics"][:, 0] = np.asarray(focal_of(sc, x), np.float64)
    return s6, np.concatenate([x[:2 * N], x[3 * N:]])


# ---- per-observation residual and Jacobians -------------------------------------------------------------------------------------
def observe_np(sc, x):
    """(r: E x 2, Jp: E x 2 x 3, Jrf: E x 2 x 4, the Jacobians with respect to w and to f side by side) in float64 at the nodes x; rows of unused
    observations are zero, and so is J_f = (p_x / p_z, p_y / p_z) on a camera whose focal length is held"""
    x = np.asarray(x, float)
    s6, x6 = _six(sc, x)
    r, Jp, Jr = R6.observe_np(s6, x6)
    rot, cam, pts = split(sc, x)
    c, t = sc["obs_cam"], sc["track_of"]
    with np.errstate(all="ignore"):
        p = np.einsum("eij,ej->ei", R6.synth.aa_to_matrix(rot)[c], pts[t] - cam[c])
        Jf = p[:, :2] / p[:, 2:]
    Jf[~(sc["used"] & sc["focal_free"][c])] = 0
    return r, Jp, np.concatenate([Jr, Jf[:, :, None]], 2)


def observe_hp(sc, x):
    """observe_np's arrays in long double, every used observation evaluated in mpmath from the input doubles"""
    x = np.asarray(x, np.float64)
    s6, x6 = _six(sc, x)
    r, Jp, Jr = R6.observe_hp(s6, x6)
    rot, cam, pts = split(sc, x)
    Jf = np.zeros((len(r), 2), LD)
    mp = B._mp
    with mpmath.workdps(MP_DPS):
        Rs = [B.rotation_mp(a) for a in rot]
        for e in np.flatnonzero(sc["used"] & sc["focal_free"][sc["obs_cam"]]):
            c, t = int(sc["obs_cam"][e]), int(sc["track_of"][e])
            _, p = B.residual_mp(Rs[c], [mp(1), mp(0), mp(0)], [mp(0), mp(0)], [mp(v) for v in pts[t]], [mp(v) for v in cam[c]])
            Jf[e] = [B._ld(p[0] / p[2]), B._ld(p[1] / p[2])]
    return r, Jp, np.concatenate([Jr, Jf[:, :, None]], 2)


def residual_hp(sc, x):
    """the plain residual (E x 2, long double) alone: for central differences"""
    s6, x6 = _six(sc, np.asarray(x, np.float64))
    return R6.observe_hp(s6, x6)[0]


# ---- Corrector, assembly (dtype of the inputs) -----------------------------------------------------------------------------------
def linearise(r, Jp, Jrf, kind=None, a=None):
    """dict(s, rho, cost, rt, Jp, Jr (E x 2 x 3), Jf (E x 2), Jc = [Jr, -Jp, Jf]: E x 2 x 7): the Corrector (ba_reference.linearise's) mixes the
    rows of every piece alike"""
    lp = B.linearise(r, Jp, kind, a)
    lr = B.linearise(r, Jrf, kind, a)["Jt"]
    return {"s": lp["s"], "rho": lp["rho"], "cost": lp["cost"], "rt": lp["rt"], "Jp": lp["Jt"], "Jr": lr[:, :, :3], "Jf": lr[:, :, 3],
            "Jc": np.concatenate([lr[:, :, :3], -lp["Jt"], lr[:, :, 3:]], axis=2)}


def assemble(sc, lin):
    """B (N x 7 x 7: w, o, f), C (T x 3 x 3), g (nodes x 3)"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    dt = lin["Jp"].dtype
    Bm, Cm, g = np.zeros((N, W, W), dt), np.zeros((T, 3, 3), dt), np.zeros((3 * N + T, 3), dt)
    c, t = sc["obs_cam"], sc["track_of"]
    np.add.at(Bm, c, np.einsum("eki,ekj->eij", lin["Jc"], lin["Jc"]))
    np.add.at(Cm, t, np.einsum("eki,ekj->eij", lin["Jp"], lin["Jp"]))
    gc = np.einsum("eki,ek->ei", lin["Jc"], lin["rt"])
    np.add.at(g, c, gc[:, :3])
    np.add.at(g, N + c, gc[:, 3:6])
    np.add.at(g[:, 0], 2 * N + c, gc[:, 6])
    np.add.at(g, 3 * N + t, np.einsum("eki,ek->ei", lin["Jp"], lin["rt"]))
    return {"B": Bm, "C": Cm, "g": g, "cost": lin["cost"]}


def cam_rows(v, N):
    """a node array's camera part (3 N x 3) as N x 7"""
    return np.concatenate([v[:N], v[N:2 * N], v[2 * N:3 * N, :1]], 1)


def cam_nodes(y7):
    """N x 7 (or 7 N) -> the 3 N camera nodes, zeros in the padding"""
    y7 = y7.reshape(-1, W)
    f = np.zeros((len(y7), 3), y7.dtype)
    f[:, 0] = y7[:, 6]
    return np.concatenate([y7[:, :3], y7[:, 3:6], f])


def node_diagonal(asm):
    d = np.einsum("kii->ki", asm["B"])
    return np.concatenate([cam_nodes(d), np.einsum("kii->ki", asm["C"])])


jacobi_scale = _over_this_layout(R6.jacobi_scale)


def damped(sc, lin, asm, S, radius, o=DEFAULTS):
    """ba6_reference.damped over 7 coordinates: D2, b (nodes x 3), Bt (N x 7 x 7), Ct, Cinv, E (per observation, 7 x 3), b7 (N x 7).  A held
    focal coordinate (zero row and column of B, no damping) and an inactive camera get the identity."""
    N = len(sc["cam_est"])
    dt = S.dtype.type
    act = active_nodes(sc)
    d = node_diagonal(asm)
    D2 = np.where(act[:, None], np.minimum(np.maximum(S * S * d, dt(o["min_lm_diagonal"])), dt(o["max_lm_diagonal"])) / dt(radius), 0)
    b = np.where(act[:, None], S * asm["g"], 0)
    S7, D7 = cam_rows(S, N), cam_rows(D2, N)
    Bt = S7[:, :, None] * asm["B"] * S7[:, None, :] + D7[:, :, None] * np.eye(W, dtype=S.dtype)
    Ct = S[3 * N:, :, None] * asm["C"] * S[3 * N:, None, :] + D2[3 * N:, :, None] * np.eye(3, dtype=S.dtype)
    Bt[~sc["cam_active"]] = np.eye(W, dtype=S.dtype)
    held = ~act[2 * N:3 * N]
    Bt[held, 6, :] = 0
    Bt[held, :, 6] = 0
    Bt[held, 6, 6] = 1
    Ct[~sc["pt_active"]] = np.eye(3, dtype=S.dtype)
    Cinv = np.array([B._inv3(m) for m in Ct]) if len(Ct) else Ct
    Cinv[~sc["pt_active"]] = 0
    E = S7[sc["obs_cam"], :, None] * np.einsum("eki,ekj->eij", lin["Jc"], lin["Jp"]) * S[3 * N + sc["track_of"], None, :]
    return B.add_cholesky(sc, {"act": act, "D2": D2, "b": b, "Bt": Bt, "Ct": Ct, "Cinv": Cinv, "E": E, "S": S, "b7": cam_rows(b, N)})


def cam_index(N, k):
    """the seven places of camera k in the flattened node vector"""
    return np.r_[3 * k:3 * k + 3, 3 * (N + k):3 * (N + k) + 3, 3 * (2 * N + k)]


def full_system(sc, dm):
    """K (3 (3N + T) square, node order) and its right-hand side; inactive rows and columns and the padding the identity, zero right-hand side"""
    N, T = len(sc["cam_est"]), len(sc["pt_est"])
    n = 3 * (3 * N + T)
    K = np.zeros((n, n), dm["S"].dtype)
    for k in range(N):
        K[np.ix_(cam_index(N, k), cam_index(N, k))] = dm["Bt"][k]
        K[3 * (2 * N + k) + 1, 3 * (2 * N + k) + 1] = K[3 * (2 * N + k) + 2, 3 * (2 * N + k) + 2] = 1
    for t in range(T):
        i = 3 * (3 * N + t)
        K[i:i + 3, i:i + 3] = dm["Ct"][t]
    for e in np.flatnonzero(sc["used"]):
        ik, it = cam_index(N, int(sc["obs_cam"][e])), 3 * (3 * N + int(sc["track_of"][e])) + np.arange(3)
        K[np.ix_(ik, it)] += dm["E"][e]
        K[np.ix_(it, ik)] += dm["E"][e].T
    return K, dm["b"].reshape(n).copy()


def schur_system(sc, dm, absolute=False):
    """ba6_reference.schur_system with 7 x 7 blocks: (Sc: 7N x 7N, rhs: 7N, Mblk: N x 7 x 7), per camera w, o, f"""
    N = len(sc["cam_est"])
    f = np.abs if absolute else (lambda z: z)
    sgn = 1 if absolute else -1
    Sc = np.zeros((W * N, W * N), dm["S"].dtype)
    Mb = f(dm["Bt"]).copy()
    rhs = f(dm["b7"]).reshape(W * N).copy()
    for k in range(N):
        Sc[W * k:W * k + W, W * k:W * k + W] = f(dm["Bt"][k])
    tp = sc["track_ptr"].astype(np.int64)
    Sc4, rhs7 = Sc.reshape(N, W, N, W).transpose(0, 2, 1, 3), rhs.reshape(N, W)
    for t in np.flatnonzero(sc["pt_active"]):
        es = np.arange(tp[t], tp[t + 1])[sc["used"][tp[t]:tp[t + 1]]]
        ks = sc["obs_cam"][es].astype(np.int64)
        Et = f(dm["E"][es])
        EC = Et @ f(dm["Cinv"][t]) if absolute or "Cchol" not in dm else B.c_solve(dm, t, np.concatenate(Et, 0).T).T.reshape(Et.shape)
        np.add.at(rhs7, ks, sgn * (EC @ f(dm["b"][3 * N + t])))
        np.add.at(Mb, ks, sgn * np.einsum("aij,akj->aik", EC, Et))
        np.add.at(Sc4, (ks[:, None], ks[None, :]), sgn * np.einsum("aij,bkj->abik", EC, Et))
    return Sc, rhs, Mb


def back_substitute(sc, dm, yc):
    """y_p = C~^-1 (b_p - E~^T y_c), T x 3; yc: 7N"""
    N = len(sc["cam_est"])
    acc = dm["b"][3 * N:].copy()
    np.add.at(acc, sc["track_of"], -np.einsum("eij,ei->ej", dm["E"], yc.reshape(N, W)[sc["obs_cam"]]))
    return np.array([B.c_solve(dm, t, acc[t]) for t in range(len(acc))]).reshape(len(acc), 3)


def solve_step(sc, lin, asm, S, radius, o=DEFAULTS, hp=False):
    """ba6_reference.solve_step: fp64 by the full system solved directly, hp by the reduced system (refined) and back-substitution"""
    dm = damped(sc, lin, asm, S, radius, o)
    if hp:
        Sc, rhs, _ = schur_system(sc, dm)
        yc = PH.solve_refined(Sc, rhs)
        return np.concatenate([cam_nodes(yc), back_substitute(sc, dm, yc)]), dm
    K, b = full_system(sc, dm)
    return np.linalg.solve(K, b).reshape(-1, 3), dm


def apply_J(sc, lin, d):
    """J~ d, E x 2: Jr d_rot + Jp (d_t - d_pos) + Jf d_f"""
    N = len(sc["cam_est"])
    c, t = sc["obs_cam"], sc["track_of"]
    return (np.einsum("eij,ej->ei", lin["Jr"], d[c]) + np.einsum("eij,ej->ei", lin["Jp"], d[3 * N + t] - d[N + c])
            + lin["Jf"] * d[2 * N + c, :1])


def gauge_directions(sc, x, jl=None):
    """ba6_reference's seven directions with a zero focal component"""
    N = len(sc["cam_est"])
    x6 = np.concatenate([x[:2 * N], x[3 * N:]])
    return [np.concatenate([v[:2 * N], np.zeros((N, 3), x.dtype), v[2 * N:]]) for v in R6.gauge_directions(sc, x6, jl)]


quad_form = _over_this_layout(R6.quad_form)
project_step = _over_this_layout(R6.project_step)
lm_solve = _over_this_layout(R6.lm_solve)   # (its result's rot, cam, points are split()'s; the focal lengths are focal_of(sc, result["x"]))


# ---- the PCG residual in the preconditioner norm and its rounding floor ------------------------------------------------------------
def _minv_norm(Mb, vec):
    v = vec.reshape(-1, W)
    return np.sqrt(sum(v[k] @ np.linalg.solve(Mb[k].astype(np.float64), v[k].astype(np.float64)) for k in range(len(v))))


pcg_residual_and_floor = _over_this_layout(R6.pcg_residual_and_floor)


def pcg_emulation(sc, dm, tol=1e-14, check=8, max_it=2000):
    """Block-Jacobi PCG in float64 on the reduced system of dm, with the looks of lm_loop.hpp's pcg_loop (every `check` iterations; a look
    is a mark when r.M^-1 r has fallen to a quarter of the last mark).  Returns (iterations or None, the longest run of iterations without a
    mark): a condition on a test's inputs -- the device's loop gives up after cg_stall_iterations (200) without a mark -- not a reference."""
    Sc, rhs, Mb = [np.asarray(v, np.float64) for v in schur_system(sc, dm)]
    Mi = np.linalg.inv(Mb)
    prec = lambda r: np.einsum("kij,kj->ki", Mi, r.reshape(-1, W)).reshape(-1)
    y, r = np.zeros_like(rhs), rhs.copy()
    z = prec(r)
    p, rz = z.copy(), r @ z
    rz0 = best = rz
    mark = longest = 0
    for it in range(1, max_it + 1):
        Ap = Sc @ p
        al = rz / (p @ Ap)
        y, r = y + al * p, r - al * Ap
        z = prec(r)
        rzn = r @ z
        p, rz = z + rzn / rz * p, rzn
        if it % check == 0:
            if np.sqrt(max(rz, 0.0) / rz0) <= tol:
                return it, longest
            if rz <= 0.25 * best:
                best, mark = rz, it
            longest = max(longest, it - mark)
    return None, longest


def aligned(sc, x, ref):
    """ba6_reference.align of the nodes x to the nodes ref, followed by the active free focal lengths (no similarity moves them)"""
    rot, cam, pts = split(sc, x)
    _, rc, rp = split(sc, ref)
    N = len(sc["cam_est"])
    return np.concatenate([align(sc, rot, cam, pts, rc, rp), focal_of(sc, x)[active_nodes(sc)[2 * N:3 * N]]])


# ---- the cases the CPU and the GPU tests share (computed once per process) ---------------------------------------------------------
LOSS = B.LOSS
CASES = {   # name: (scene, sigma, seed, relative sigma of the focal lengths[, loss: default LOSS]); chosen on the CPU: tests/test_ba7_reference.py asserts the conditions
    "a_near": ("a", 0.05, 1, 0.01), "a_far": ("a", 2.0, 4, 0.05), "b_near": ("b", 0.05, 1, 0.01), "b_far": ("b", 1.0, 1, 0.05),
    "c_near": ("c", 0.05, 1, 0.01), "c_far": ("c", 2.0, 3, 0.05), "t_near": ("t", 0.05, 1, 0.01), "t_far": ("t", 1.0, 5, 0.05),
    "t_near_tukey": ("t", 0.05, 1, 0.01, B.TUKEY), "a_near_tukey": ("a", 0.05, 1, 0.01, B.TUKEY), "a_near_geman": ("a", 0.05, 1, 0.01, B.GEMAN),
}


def near_start(sname):
    return nodes(*perturbed_start(scene("b" if sname == "t" else sname), *NEAR))   # (t is b's geometry with other observations)


def case_loss(name):
    return CASES[name][4] if len(CASES[name]) > 4 else LOSS


def case_start(name):
    sname, sigma, seed, sf = CASES[name][:4]
    return nodes(*perturbed_start(scene(sname), sigma, seed, sf))


def case_solve(name, hp):
    return cached(("solve7", name, hp), lambda: lm_solve(scene(CASES[name][0]), case_start(name), *case_loss(name), hp=hp))


def point_observation(sname, hp, focal_free=None):
    key = None if focal_free is None else bytes(np.asarray(focal_free, np.uint8))
    return cached(("obs7", sname, hp, key), lambda: (observe_hp if hp else observe_np)(scene(sname, focal_free), near_start(sname)))


def point_linearisation(sname, kind, a, hp, focal_free=None):
    """(lin, asm) at the near start of the scene"""
    key = None if focal_free is None else bytes(np.asarray(focal_free, np.uint8))

    def make():
        lin = linearise(*point_observation(sname, hp, focal_free), kind, a)
        return lin, assemble(scene(sname, focal_free), lin)
    return cached(("lin7", sname, kind, a, hp, key), make)
