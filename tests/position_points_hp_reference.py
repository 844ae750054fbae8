"""High-precision reference of position estimation with point-to-camera constraints (include/gsfm_posp.h); test helper, not a conftest.

Tier 1 (mpmath, position_hp_reference's 50 digits).  The ray of an observation, normalise(R(aa_k)^T ((x - u) / f, (y - v) / f, 1)), from
the exact input doubles with the exact rotation; the residual w_p ((X - c) / n - ray) with the guard decided on the exact n; its Jacobian
with respect to the point by central differences (position_hp_reference.edge_linearise: nothing relies on the closed form).

Tier 2 (numpy longdouble).  The joint graph of cameras and points -- the view-graph edges, then one edge (camera k, node N + t) per used
observation -- in hp_reference's per-edge layout, so that hp_reference.corrected / assemble / matvec and position_hp_reference.corrected
apply unchanged.  Error scales extended by w_p: e_mag = w_p (1 + |ray|) = 2 w_p and Jw = 2 w_p / n for an observation.

The systems of one LM step are assembled by functions that take the number format as an argument, so that the float64 tier
(tests/position_points_reference.py's closed forms evaluated in float64) and the long-double tier run the same steps: the joint normal
matrix, the damped scaled system of the full problem, the explicit Schur complement on the cameras, the step from the FULL system, its
gauge projection and the model cost change.
"""
import mpmath
import numpy as np

import hp_reference as H
import position_hp_reference as PH
import position_points_reference as PR

LD = H.LD
U = H.U


def ray_mp(aa, K, xy):
    """the unit ray in mpmath (list of 3)"""
    f, u, v = (PH._mp(k) for k in K)
    t = [(PH._mp(xy[0]) - u) / f, (PH._mp(xy[1]) - v) / f, mpmath.mpf(1)]
    w = [PH._mp(x) for x in aa]   # (position_hp_reference.direction rounds its vector to a double first: restated for the mpmath t)
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if th2 == 0:
        d = t
    else:
        th = mpmath.sqrt(th2)
        k = [x / th for x in w]
        ct, st = mpmath.cos(th), mpmath.sin(th)
        kt = k[0] * t[0] + k[1] * t[1] + k[2] * t[2]
        cross = [k[1] * t[2] - k[2] * t[1], k[2] * t[0] - k[0] * t[2], k[0] * t[1] - k[1] * t[0]]
        d = [t[c] * ct - cross[c] * st + k[c] * kt * (1 - ct) for c in range(3)]   # R^T t: the rotation by -theta
    n = mpmath.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
    return [x / n for x in d]


def joint_edge_set(sc, cam_pos, points, weight):
    """Tier 1 over the joint graph at (cam_pos, points): hp_reference's per-edge dict (r, Ji, Jj, e_mag, Jw_i, Jw_j, d, n, unit) with the
    weight applied, plus ei, ej (joint node indices), n_nodes, n_edges (view-graph edges come first), used (per observation) and ray
    (n_obs x 3 long double, zeros where the observation is not used)."""
    N = int(sc["n_cams"])
    st = PR.structure(N, sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    used = st["used"]
    T = len(st["point_active"])
    E = len(sc["edge_i"])
    cam_pos = np.asarray(cam_pos, np.float64).reshape(N, 3)
    points = np.asarray(points, np.float64).reshape(T, 3)
    ref = PH.edge_set(sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], cam_pos)
    oc = np.asarray(sc["obs_cam"], np.int64)
    xy = np.asarray(sc["obs_xy"], np.float64).reshape(-1, 2)
    idx = np.flatnonzero(used)
    M = len(idx)
    ob = {"r": np.zeros((M, 3), LD), "Ji": np.zeros((M, 3, 3), LD), "Jj": np.zeros((M, 3, 3), LD), "e_mag": np.zeros((M, 3), LD),
          "Jw_i": np.zeros((M, 3), LD), "Jw_j": np.zeros((M, 3), LD), "d": np.zeros((M, 3), LD), "n": np.zeros(M, LD), "unit": np.zeros(M, bool)}
    w = float(weight)
    ray = np.zeros((len(used), 3), LD)
    with mpmath.workdps(PH.MP_DPS):
        wm = PH._mp(w)
        for m, e in enumerate(idx):
            k, t = int(oc[e]), int(st["track_of"][e])
            d = ray_mp(sc["ray_rot_aa"][k], sc["intrinsics"][k], xy[e])
            r, J, n, unit = PH.edge_linearise(cam_pos[k], points[t], d)
            ob["r"][m] = [PH._ld(wm * x) for x in r]
            P = np.array([[PH._ld(wm * x) for x in row] for row in J], dtype=LD)
            ob["Jj"][m], ob["Ji"][m] = P, -P
            ob["d"][m] = ray[e] = [PH._ld(x) for x in d]
            ob["n"][m], ob["unit"][m] = PH._ld(n), unit
            ob["e_mag"][m] = 2.0 * w
            if unit:
                ob["Jw_i"][m] = ob["Jw_j"][m] = 2.0 * w / float(n)
    out = {k: np.concatenate([ref[k], ob[k]]) for k in ob}
    out.update(ei=np.concatenate([np.asarray(sc["edge_i"], np.int64), oc[idx]]), ej=np.concatenate([np.asarray(sc["edge_j"], np.int64), N + st["track_of"][idx]]),
               n_nodes=N + T, n_edges=E, used=used, ray=ray, structure=st)
    return out


# ---- the systems of one LM step, in the number format `dt` ----------------------------------------------------------------------------
def normal_system(A, rt, ei, ej, n_nodes, dt):
    """(L, g): the joint normal matrix J~^T J~ (3n x 3n: +H on an edge's two diagonal blocks, -H off the diagonal) and the gradient
    (3n) from the corrected far-end Jacobians A (E x 3 x 3) and the corrected residuals rt, summed in `dt`"""
    A, rt = np.asarray(A, dt), np.asarray(rt, dt)
    Hs = np.einsum("eki,ekj->eij", A, A)
    ge = np.einsum("ekc,ek->ec", A, rt)
    L = np.zeros((3 * n_nodes, 3 * n_nodes), dt)
    g = np.zeros((n_nodes, 3), dt)
    for e, (i, j) in enumerate(zip(ei, ej)):
        si, sj = slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3)
        L[si, si] += Hs[e]; L[sj, sj] += Hs[e]; L[si, sj] -= Hs[e]; L[sj, si] -= Hs[e]
        g[j] += ge[e]; g[i] -= ge[e]
    return L, g.reshape(-1)


def damped_system(L, g, active, radius, dt, min_diag=1e-6, max_diag=1e32, jacobi=True):
    """position_hp_reference.step_system's rules in `dt`: S, D2, K = S L S + D2 and b = S g; inactive rows and columns the identity, b = 0"""
    n = L.shape[0]
    dg = np.diagonal(L).copy()
    S = (1 / (1 + np.sqrt(dg))) if jacobi else np.ones(n, dt)
    act = np.repeat(np.asarray(active, bool), 3)
    D2 = np.minimum(np.maximum(S * S * dg, dt(min_diag)), dt(max_diag)) / dt(radius)
    K = S[:, None] * L * S[None, :] + np.diag(D2)
    off = np.flatnonzero(~act)
    K[off, :] = 0
    K[:, off] = 0
    K[off, off] = 1
    return {"L": L, "g": g, "S": S, "D2": np.where(act, D2, 0), "K": K, "b": np.where(act, S * g, 0), "act": act}


def _inv3(M):
    return H.sym3_inverse(M) if M.dtype == LD else np.linalg.inv(M)


def schur_system(sysm, n_cams):
    """(Sc, rhs, Mblocks): the explicit Schur complement K_cc - K_cp K_pp^-1 K_pc on the cameras (K_pp is block diagonal: one 3 x 3 per
    point), the reduced right-hand side and the 3 x 3 diagonal blocks of Sc (the preconditioner)"""
    K, b = sysm["K"], sysm["b"]
    c = 3 * n_cams
    T = (K.shape[0] - c) // 3
    Kcc, Kcp, bp = K[:c, :c], K[:c, c:], b[c:]
    if T == 0:
        Sc, rhs = Kcc.copy(), b[:c].copy()
    else:
        Cinv = _inv3(np.stack([K[c + 3 * t:c + 3 * t + 3, c + 3 * t:c + 3 * t + 3] for t in range(T)]))
        W = np.concatenate([Kcp[:, 3 * t:3 * t + 3] @ Cinv[t] for t in range(T)], axis=1)   # K_cp K_pp^-1
        Sc, rhs = Kcc - W @ Kcp.T, b[:c] - W @ bp
    Mb = np.stack([Sc[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(n_cams)])
    return Sc, rhs, Mb


def solve_full(sysm):
    """y of the FULL damped system K y = b (cameras and points together; nothing eliminated)"""
    if sysm["K"].dtype == LD:
        return PH.solve_refined(sysm["K"], sysm["b"])
    return np.linalg.solve(sysm["K"], sysm["b"])


def back_substitute(sysm, n_cams, yc):
    """y_p = K_pp^-1 (b_p - K_pc y_c)"""
    K, b = sysm["K"], sysm["b"]
    c = 3 * n_cams
    T = (K.shape[0] - c) // 3
    t = b[c:] - K[c:, :c] @ np.asarray(yc, K.dtype).reshape(-1)
    Cinv = _inv3(np.stack([K[c + 3 * k:c + 3 * k + 3, c + 3 * k:c + 3 * k + 3] for k in range(T)]))
    return np.einsum("tab,tb->ta", Cinv, t.reshape(T, 3))


def project_step(sysm, y, x, fixed, gauge=True):
    """(delta, model cost change): delta = -S y on active rows, its component along v = x - x_fixed over the active nodes removed"""
    dt = sysm["K"].dtype
    act = sysm["act"]
    delta = np.where(act, -sysm["S"] * y, 0)
    xx = np.asarray(x, dt).reshape(-1)
    if gauge and fixed >= 0:
        v = np.where(act, xx - np.tile(xx[3 * fixed:3 * fixed + 3], len(xx) // 3), 0)
        vv = v @ v
        if vv > 0:
            delta = delta - (delta @ v / vv) * v
    return delta, -(delta @ sysm["g"]) - (delta @ (sysm["L"] @ delta)) / 2


def first_pcg_iterate(Sc, rhs, Mb):
    """PCG's first iterate from zero: y1 = alpha z, z = M^-1 rhs, alpha = rhs.z / z.Sc z"""
    z = np.einsum("kab,kb->ka", _inv3(Mb), rhs.reshape(-1, 3)).reshape(-1)
    return (rhs @ z) / (z @ (Sc @ z)) * z
