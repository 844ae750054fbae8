"""A numpy / scipy restatement of the robust L1 + IRLS rotation estimator as include/gsfm_rot_l1l2.h defines it (Theia's ROBUST_L1L2),
written from that definition.  linear="direct": every linear system by a sparse LU; linear="pcg": by Jacobi PCG in numpy with the
library's stopping quantity sqrt(r.M^-1 r / b.M^-1 b), looked at after every iteration.

solve() returns the rotations and a log: the ADMM iterations and avg of every outer iteration, the IRLS iterations with their avg, the
PCG iterations, and the decision margin: the smallest relative distance |q - t| / t of any compared quantity q from its threshold t --
the two ADMM tests at every ADMM iteration, avg at every outer and every IRLS iteration.  A graph whose margin is far above the
agreement of two implementations takes the same decisions in both."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

DEFAULTS = dict(max_num_l1_iterations=5, max_num_irls_iterations=100, l1_step_convergence_threshold=1e-3, irls_step_convergence_threshold=1e-3,
                irls_loss_parameter_sigma=5.0 * np.pi / 180.0, admm_initial_iterations=5, admm_rho=1.0, admm_alpha=1.0, admm_absolute_tolerance=1e-4,
                admm_relative_tolerance=1e-2, max_cg_iterations=2000, cg_relative_tolerance=1e-14)


def aa_to_quat(aa):
    """Ceres' AngleAxisToQuaternion, (x, y, z, w)"""
    aa = np.asarray(aa, dtype=np.float64)
    t2 = np.sum(aa * aa, axis=-1, keepdims=True)
    t = np.sqrt(t2)
    safe = np.where(t2 > 0.0, t, 1.0)
    k = np.where(t2 > 0.0, np.sin(0.5 * safe) / safe, 0.5)
    w = np.where(t2 > 0.0, np.cos(0.5 * safe), 1.0)
    return np.concatenate([aa * k, w], axis=-1)


def quat_to_aa(q):
    """Ceres' QuaternionToAngleAxis: the angle in (-pi, pi]"""
    q = np.asarray(q, dtype=np.float64)
    v, w = q[..., :3], q[..., 3:4]
    s2 = np.sum(v * v, axis=-1, keepdims=True)
    s = np.sqrt(s2)
    two_theta = 2.0 * np.where(w < 0.0, np.arctan2(-s, -w), np.arctan2(s, w))
    k = np.where(s2 > 0.0, two_theta / np.where(s2 > 0.0, s, 1.0), 2.0)
    return v * k


def quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def quat_conj(a):
    return a * np.array([-1.0, -1.0, -1.0, 1.0])


def residuals(edge_i, edge_j, rel_aa, rot_aa):
    """b_e = Log(R_j^T R_ij R_i), E x 3"""
    q = aa_to_quat(rot_aa)
    return _residuals_q(np.asarray(edge_i), np.asarray(edge_j), aa_to_quat(rel_aa), q)


def _residuals_q(ei, ej, qrel, q):
    return quat_to_aa(quat_mul(quat_conj(q[ej]), quat_mul(qrel, q[ei])))


def incidence(n_cams, edge_i, edge_j, fixed_cam):
    """(B, free): the signed E x (N - 1) edge-camera incidence matrix over the free cameras (those with an edge, less fixed_cam, ascending)"""
    ei, ej = np.asarray(edge_i, dtype=np.int64), np.asarray(edge_j, dtype=np.int64)
    present = np.zeros(n_cams, dtype=bool)
    present[ei] = True; present[ej] = True
    if not present[fixed_cam]:
        raise ValueError("fixed_cam appears in no edge")
    free = np.flatnonzero(present & (np.arange(n_cams) != fixed_cam))
    col = -np.ones(n_cams, dtype=np.int64)
    col[free] = np.arange(free.shape[0])
    E = ei.shape[0]
    rows = np.concatenate([np.arange(E), np.arange(E)])
    cols = np.concatenate([col[ej], col[ei]])
    vals = np.concatenate([np.ones(E), -np.ones(E)])
    keep = cols >= 0
    B = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(E, free.shape[0]))
    return B, free


def pcg(L, rhs, tol, max_iterations):
    """Jacobi PCG on L x = rhs (rhs: n x 3, one recurrence over all 3 n entries) from x = 0.  Returns (x, iterations, sqrt(rz / rz0))."""
    d = L.diagonal()[:, None]
    x = np.zeros_like(rhs)
    r = rhs.copy()
    z = r / d
    p = z.copy()
    rz = rz0 = float(np.sum(r * z))
    if rz0 == 0.0:
        return x, 0, 0.0
    rel = 1.0
    for it in range(1, max_iterations + 1):
        Ap = L @ p
        alpha = rz / float(np.sum(p * Ap))
        x += alpha * p
        r -= alpha * Ap
        z = r / d
        rz_new = float(np.sum(r * z))
        rel = np.sqrt(max(rz_new, 0.0) / rz0)
        if rel <= tol:
            return x, it, rel
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_iterations, rel


def laplacian_solve(n_cams, edge_i, edge_j, rhs, weights=None, fixed_cam=0, linear="direct", cg_relative_tolerance=DEFAULTS["cg_relative_tolerance"],
                    max_cg_iterations=2000):
    """x = L_w^-1 rhs on the free cameras (n_cams x 3, zero elsewhere); returns (x, PCG iterations, final relative residual)"""
    B, free = incidence(n_cams, edge_i, edge_j, fixed_cam)
    w = np.ones(B.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    L = (B.T @ sp.diags(w) @ B).tocsr()
    b = np.asarray(rhs, dtype=np.float64).reshape(n_cams, 3)[free]
    if linear == "direct":
        xf, it, rel = spla.splu(L.tocsc()).solve(b), 0, 0.0
    elif linear == "dense":
        xf, it, rel = np.linalg.solve(L.toarray(), b), 0, 0.0
    else:
        xf, it, rel = pcg(L, b, cg_relative_tolerance, max_cg_iterations)
    x = np.zeros((n_cams, 3))
    x[free] = xf
    return x, it, rel


def solve(n_cams, edge_i, edge_j, rel_aa, init_aa, fixed_cam=0, linear="direct", **options):
    o = dict(DEFAULTS)
    for k, v in options.items():
        if k not in o:
            raise TypeError("unknown option %r" % k)
        o[k] = v
    ei, ej = np.asarray(edge_i, dtype=np.int64), np.asarray(edge_j, dtype=np.int64)
    init = np.asarray(init_aa, dtype=np.float64).reshape(n_cams, 3)
    B, free = incidence(n_cams, ei, ej, fixed_cam)
    E, nf = B.shape
    Bt = B.T.tocsr()
    q = aa_to_quat(init)
    qrel = aa_to_quat(np.asarray(rel_aa, dtype=np.float64).reshape(E, 3))
    touched = np.zeros(n_cams, dtype=bool)
    log = {"admm_iterations": [], "l1_step": [], "irls_iterations": 0, "irls_step": [], "cg_iterations": 0, "margin": np.inf,
           "l1_converged": False, "irls_converged": False}

    def compare(value, threshold):
        if threshold > 0.0:
            log["margin"] = min(log["margin"], abs(value - threshold) / threshold)

    def solver_for(L):
        if linear == "direct":
            lu = spla.splu(L.tocsc())
            return lambda b: lu.solve(b)
        if linear == "dense":
            Ld = L.toarray()
            return lambda b: np.linalg.solve(Ld, b)

        def run(b):
            x, it, _ = pcg(L, b, o["cg_relative_tolerance"], o["max_cg_iterations"])
            log["cg_iterations"] += it
            return x
        return run

    def update(x):
        step = np.linalg.norm(x, axis=1)
        moved = step > 0.0
        k = free[moved]
        qn = quat_mul(q[k], aa_to_quat(x[moved]))
        q[k] = qn / np.linalg.norm(qn, axis=1, keepdims=True)
        touched[k] = True
        return float(np.sum(step)) / nf

    b = _residuals_q(ei, ej, qrel, q)
    # ---- L1 stage
    rho, alpha = o["admm_rho"], o["admm_alpha"]
    solve_l1 = solver_for((Bt @ B).tocsr())
    inner = o["admm_initial_iterations"]
    for _ in range(o["max_num_l1_iterations"]):
        z = np.zeros((E, 3)); u = np.zeros((E, 3)); x = np.zeros((nf, 3))
        it = 0
        while it < inner:
            x = solve_l1(Bt @ (b + z - u))
            ax = B @ x
            h = alpha * ax + (1.0 - alpha) * (z + b)
            z_old = z
            a = h - b + u
            z = np.maximum(0.0, a - 1.0 / rho) - np.maximum(0.0, -a - 1.0 / rho)
            u = u + (h - z - b)
            it += 1
            r_norm = np.linalg.norm(ax - z - b)
            s_norm = np.linalg.norm(rho * (Bt @ (z - z_old)))
            eps_pri = np.sqrt(3.0 * E) * o["admm_absolute_tolerance"] + o["admm_relative_tolerance"] * max(np.linalg.norm(ax), np.linalg.norm(z), np.linalg.norm(b))
            eps_dual = np.sqrt(3.0 * nf) * o["admm_absolute_tolerance"] + o["admm_relative_tolerance"] * np.linalg.norm(rho * (Bt @ u))
            compare(r_norm, eps_pri); compare(s_norm, eps_dual)
            if r_norm < eps_pri and s_norm < eps_dual:
                break
        avg = update(x)
        b = _residuals_q(ei, ej, qrel, q)
        log["admm_iterations"].append(it); log["l1_step"].append(avg)
        compare(avg, o["l1_step_convergence_threshold"])
        if avg <= o["l1_step_convergence_threshold"]:
            log["l1_converged"] = True
            break
        inner *= 2
    # ---- IRLS stage
    sigma = o["irls_loss_parameter_sigma"]
    for it in range(o["max_num_irls_iterations"]):
        t = np.sum(b * b, axis=1) + sigma * sigma
        w = sigma / (t * t)
        W = sp.diags(w)
        x = solver_for((Bt @ W @ B).tocsr())(Bt @ (w[:, None] * b))
        avg = update(x)
        b = _residuals_q(ei, ej, qrel, q)
        log["irls_iterations"] = it + 1; log["irls_step"].append(avg)
        compare(avg, o["irls_step_convergence_threshold"])
        if avg < o["irls_step_convergence_threshold"]:
            log["irls_converged"] = True
            break
    rot = init.copy()
    rot[touched] = quat_to_aa(q[touched])
    return rot, log


def relative_to_fixed_error_deg(rot_aa, gt_aa, fixed_cam):
    """Per-camera angle (degrees) between R_k R_fixed^T of the estimate and of the ground truth: no alignment"""
    def rel(aa):
        qq = aa_to_quat(aa)
        return quat_mul(qq, quat_conj(qq[fixed_cam:fixed_cam + 1]))
    d = quat_mul(rel(np.asarray(rot_aa)), quat_conj(rel(np.asarray(gt_aa))))
    return np.degrees(2.0 * np.arctan2(np.linalg.norm(d[:, :3], axis=1), np.abs(d[:, 3])))


def theia_case(n_views, n_pairs, noise_deg, seed):
    """A case as Theia's robust_rotation_estimator_test.cc builds one: random orientations, a chain (k - 1, k) and random further pairs,
    rotation_2 = R_j R_i^T with a rotation of noise_deg about a random axis applied, the start composed along the chain from the first
    view's true orientation.  Returns dict(n_cams, edge_i, edge_j, rel_aa, gt_aa, init_aa)."""
    rng = np.random.default_rng(seed)
    gt_q = aa_to_quat(rng.uniform(-1.0, 1.0, (n_views, 3)))
    pairs = [(k - 1, k) for k in range(1, n_views)]
    have = set(pairs)
    while len(pairs) < n_pairs:
        i, j = sorted(int(v) for v in rng.integers(0, n_views, 2))
        if i != j and (i, j) not in have:
            have.add((i, j)); pairs.append((i, j))
    ei = np.array([p[0] for p in pairs], dtype=np.uint32); ej = np.array([p[1] for p in pairs], dtype=np.uint32)
    qrel = quat_mul(gt_q[ej], quat_conj(gt_q[ei]))
    if noise_deg > 0.0:
        axis = rng.standard_normal((len(pairs), 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        qrel = quat_mul(aa_to_quat(axis * np.radians(noise_deg)), qrel)
    rel_aa = quat_to_aa(qrel)
    init_q = gt_q.copy()
    for k in range(1, n_views):   # the chain's edges are the first n_views - 1
        init_q[k] = quat_mul(aa_to_quat(rel_aa[k - 1]), init_q[k - 1])
    return {"n_cams": n_views, "edge_i": ei, "edge_j": ej, "rel_aa": np.ascontiguousarray(rel_aa), "gt_aa": quat_to_aa(gt_q),
            "init_aa": np.ascontiguousarray(quat_to_aa(init_q))}
