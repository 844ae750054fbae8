"""Seeded synthetic pose graphs and the evaluation metric.

numpy only (PCG64 generator: platform independent); no device code.  Conventions are the
reference's: world->camera angle-axis per camera, R_ij = R_j R_i^T on edge (i, j), i < j.
"""
import numpy as np


# ---- small vectorised SO(3) toolkit (quaternions as [..., (x, y, z, w)]) ----
def aa_to_quat(aa):
    aa = np.asarray(aa, dtype=np.float64)
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    small = th < 1e-12
    k = np.where(small, 0.5, np.sin(0.5 * th) / np.where(small, 1.0, th))
    return np.concatenate([aa * k, np.where(small, 1.0, np.cos(0.5 * th))], axis=-1)


def quat_to_aa(q):
    q = np.asarray(q, dtype=np.float64)
    v, w = q[..., :3], q[..., 3:4]
    s = np.linalg.norm(v, axis=-1, keepdims=True)
    sign = np.where(w < 0, -1.0, 1.0)
    two_theta = 2.0 * np.arctan2(sign * s, sign * w)
    k = np.where(s > 0, two_theta / np.where(s > 0, s, 1.0), 2.0)
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


def quat_to_matrix(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def random_unit_quat(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def make_edges(rng, n_cams, n_edges):
    """Spanning chain (k-1, k) plus uniformly random distinct pairs i < j."""
    if n_edges < n_cams - 1:
        raise ValueError("need at least n_cams - 1 edges")
    max_edges = n_cams * (n_cams - 1) // 2
    if n_edges > max_edges:
        raise ValueError("more edges than distinct pairs")
    chain_i = np.arange(0, n_cams - 1, dtype=np.int64)
    chain_j = chain_i + 1
    key_chain = chain_i * n_cams + chain_j
    need = n_edges - (n_cams - 1)
    keys = np.empty(0, dtype=np.int64)
    while keys.size < need:
        m = int((need - keys.size) * 1.2) + 16
        a = rng.integers(0, n_cams, m)
        b = rng.integers(0, n_cams, m)
        ok = (a != b) & (np.abs(a - b) != 1)
        lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
        keys = np.unique(np.concatenate([keys, lo * n_cams + hi]))
        if keys.size > need:
            keys = rng.permutation(keys)[:need]
    keys = np.concatenate([key_chain, np.sort(keys)])
    return (keys // n_cams).astype(np.uint32), (keys % n_cams).astype(np.uint32)


def make_local_edges(rng, n_cams, n_edges, window, shuffle=True):
    """A spatially coherent view graph with arbitrary ids: in a hidden ordering every camera is linked to its successor
    and to random cameras at most window/2 places away; the ids are then shuffled (shuffle=True), which is how real
    datasets arrive.  Returns (edge_i, edge_j) with edge_i < edge_j."""
    chain_i = np.arange(0, n_cams - 1, dtype=np.int64)
    need = n_edges - (n_cams - 1)
    # pairs (a, a + d) with 2 <= d <= window // 2 (d >= 2: the chain holds d = 1) and a + d < n_cams
    reach = max(2, window // 2)
    available = sum(max(0, n_cams - d) for d in range(2, reach + 1))
    if need > available:
        raise ValueError("a window of %d admits only %d edges beside the chain on %d cameras, %d asked for" % (window, available, n_cams, need))
    keys = np.empty(0, dtype=np.int64)
    while keys.size < need:
        m = int((need - keys.size) * 1.3) + 16
        a = rng.integers(0, n_cams, m)
        b = a + rng.integers(2, max(3, window // 2 + 1), m)
        ok = b < n_cams
        keys = np.unique(np.concatenate([keys, a[ok] * n_cams + b[ok]]))
        if keys.size > need:
            keys = rng.permutation(keys)[:need]
    keys = np.concatenate([chain_i * n_cams + chain_i + 1, np.sort(keys)])
    i, j = keys // n_cams, keys % n_cams
    if shuffle:
        sigma = rng.permutation(n_cams)
        i, j = sigma[i], sigma[j]
    return np.minimum(i, j).astype(np.uint32), np.maximum(i, j).astype(np.uint32)


def make_graph(n_cams, n_edges, seed, outlier_frac=0.0, scale=0.2, full_so3=False,
               sigma_deg=(0.2, 2.0), kappa=3e-4, init_noise_deg=2.0, noise=True, local_window=0):
    """Returns dict(n_cams, edge_i, edge_j, rel_aa, cov6, inlier_weight, gt_aa, init_aa, is_outlier).

    Inlier measurement R_ij = Exp(n) R_j R_i^T with n ~ N(0, Sigma_ij), Sigma_ij = A diag(s^2) A^T,
    s ~ logU[sigma_deg]; the covariance handed to the solver is kappa * Sigma_ij so that the whitened
    inlier s_e = 1e-8 n^T (kappa Sigma)^-1 n averages 1e-4 (MAGSAC sigma_max = 0.02 scale).
    Outliers (only among the non-chain edges) are uniform random rotations.  The initial guess is the
    ground truth perturbed by init_noise_deg (stand-in for the spanning-tree initialisation).
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    if full_so3:
        q_gt = random_unit_quat(rng, n_cams)
        gt_aa = quat_to_aa(q_gt)
    else:
        gt_aa = scale * rng.uniform(-1.0, 1.0, (n_cams, 3))
    q_gt = aa_to_quat(gt_aa)
    ei, ej = make_local_edges(rng, n_cams, n_edges, local_window) if local_window else make_edges(rng, n_cams, n_edges)
    E = ei.shape[0]
    q_rel = quat_mul(q_gt[ej], quat_conj(q_gt[ei]))
    lo, hi = np.log(np.deg2rad(sigma_deg[0])), np.log(np.deg2rad(sigma_deg[1]))
    sig = np.exp(rng.uniform(lo, hi, (E, 3)))
    q_axes = random_unit_quat(rng, E)
    z = rng.standard_normal((E, 3)) if noise else None
    # the 3x3 intermediates (axes, covariance) are the bulk of the memory: built in blocks of edges, so that the 80M-edge graph
    # of an 8-rank weak-scaling run peaks at ~12 GB per rank instead of ~30 GB
    cov6 = np.empty((E, 6))
    n = np.empty((E, 3)) if noise else None
    for b0 in range(0, E, 1 << 22):
        sl = slice(b0, min(E, b0 + (1 << 22)))
        A = quat_to_matrix(q_axes[sl])
        Sf = kappa * np.einsum("eij,ej,ekj->eik", A, sig[sl] * sig[sl], A)
        cov6[sl] = np.stack([Sf[:, 0, 0], Sf[:, 1, 1], Sf[:, 2, 2], Sf[:, 0, 1], Sf[:, 0, 2], Sf[:, 1, 2]], axis=1)
        if noise:
            n[sl] = np.einsum("eij,ej->ei", A, sig[sl] * z[sl])
    del q_axes, z
    if noise:
        q_rel = quat_mul(aa_to_quat(n), q_rel)
    is_out = np.zeros(E, dtype=bool)
    if outlier_frac > 0:
        cand = np.arange(n_cams - 1, E)   # (with local_window the chain is not a prefix of the shuffled list: any edge may be hit)
        k = int(round(outlier_frac * E))
        pick = rng.choice(cand, size=min(k, cand.size), replace=False)
        is_out[pick] = True
        q_rel[pick] = random_unit_quat(rng, pick.size)
    init_q = quat_mul(aa_to_quat(np.deg2rad(init_noise_deg) * rng.standard_normal((n_cams, 3))), q_gt)
    inlier_weight = rng.integers(30, 400, E).astype(np.float64) / 100.0
    return {"n_cams": int(n_cams), "edge_i": ei, "edge_j": ej, "rel_aa": np.ascontiguousarray(quat_to_aa(q_rel)),
            "cov6": np.ascontiguousarray(cov6), "inlier_weight": inlier_weight, "gt_aa": gt_aa,
            "init_aa": np.ascontiguousarray(quat_to_aa(init_q)), "is_outlier": is_out}


def spanning_tree_init(g, seed=0, inlier_matches=(150, 1500), outlier_matches=(16, 150)):
    """The initialisation the reference pipeline feeds the solver (OrientationsFromMaximumSpanningTree, Theia
    orientations_from_maximum_spanning_tree.cc:62-181): a maximum spanning tree of the view graph weighted by the number of verified
    matches, rotations composed from the root along the tree (R_j = R_ij R_i going up in id, R_i = R_ij^T R_j going down).  Match
    counts are drawn so that inlier edges dominate the tree, as they do in real view graphs (an outlier pair has few verified matches).
    Returns (init_aa, num_matches).  SURVEY 8(d): "Init = chain composition or BFS-tree composition"."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, minimum_spanning_tree
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    n, ei, ej = g["n_cams"], g["edge_i"].astype(np.int64), g["edge_j"].astype(np.int64)
    E = ei.size
    m = rng.integers(inlier_matches[0], inlier_matches[1], E)
    out = g["is_outlier"]
    m[out] = rng.integers(outlier_matches[0], outlier_matches[1], int(out.sum()))
    tree = minimum_spanning_tree(sp.coo_matrix((-m.astype(np.float64), (ei, ej)), shape=(n, n)).tocsr())
    order, pred = breadth_first_order(tree + tree.T, 0, directed=False)
    order, pred = order.astype(np.int64), pred.astype(np.int64)   # (scipy returns int32: lo * n + hi below would overflow from 46k cameras on)
    keys = ei * n + ej
    srt = np.argsort(keys, kind="stable")
    q_rel = aa_to_quat(g["rel_aa"])
    q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))      # cameras outside the root's component keep the identity
    depth = np.zeros(n, dtype=np.int64)
    nodes = order[1:]
    for v in nodes:                                            # (BFS order: a parent's depth is final before its children are visited)
        depth[v] = depth[pred[v]] + 1
    for d in range(1, int(depth.max()) + 1 if nodes.size else 1):
        v = nodes[depth[nodes] == d]
        p = pred[v]
        lo, hi = np.minimum(p, v), np.maximum(p, v)
        e = srt[np.searchsorted(keys, lo * n + hi, sorter=srt)]
        up = p < v                                             # the parent is `first`: R_v = R_ij R_p; else R_v = R_ij^T R_p
        q[v] = np.where(up[:, None], quat_mul(q_rel[e], q[p]), quat_mul(quat_conj(q_rel[e]), q[p]))
    return np.ascontiguousarray(quat_to_aa(q)), m


def angular_distance(aa_a, aa_b):
    """Per-camera geodesic distance (rad) between two sets of rotations, no alignment."""
    q = quat_mul(aa_to_quat(aa_a), quat_conj(aa_to_quat(aa_b)))
    return 2.0 * np.arctan2(np.linalg.norm(q[..., :3], axis=-1), np.abs(q[..., 3]))


def align_rotations(aa_est, aa_ref):
    """Global gauge alignment est * R = ref (AlignRotations semantics, Theia align_rotations.cc:132-154):
    chordal L2 mean of R_est^T R_ref projected on SO(3). Returns the aligned angle-axis set."""
    Re = quat_to_matrix(aa_to_quat(aa_est))
    Rr = quat_to_matrix(aa_to_quat(aa_ref))
    M = np.einsum("nji,njk->ik", Re, Rr)
    U, _, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    Ra = Re @ R
    # matrix -> quaternion via the robust trace method, vectorised through scipy-free eigen trick
    q = matrix_to_quat(Ra)
    return quat_to_aa(q)


def matrix_to_quat(R):
    R = np.asarray(R)
    m00, m11, m22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    q = np.empty(R.shape[:-2] + (4,))
    tr = m00 + m11 + m22
    c0 = tr >= 0
    c1 = (~c0) & (m00 >= m11) & (m00 >= m22)
    c2 = (~c0) & (~c1) & (m11 >= m22)
    c3 = (~c0) & (~c1) & (~c2)
    t = np.sqrt(np.maximum(np.where(c0, 1 + tr, np.where(c1, 1 + m00 - m11 - m22, np.where(c2, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22))), 1e-300))
    s = 0.5 / t
    q[..., 3] = np.where(c0, 0.5 * t, np.where(c1, (R[..., 2, 1] - R[..., 1, 2]) * s, np.where(c2, (R[..., 0, 2] - R[..., 2, 0]) * s, (R[..., 1, 0] - R[..., 0, 1]) * s)))
    q[..., 0] = np.where(c0, (R[..., 2, 1] - R[..., 1, 2]) * s, np.where(c1, 0.5 * t, np.where(c2, (R[..., 0, 1] + R[..., 1, 0]) * s, (R[..., 0, 2] + R[..., 2, 0]) * s)))
    q[..., 1] = np.where(c0, (R[..., 0, 2] - R[..., 2, 0]) * s, np.where(c1, (R[..., 0, 1] + R[..., 1, 0]) * s, np.where(c2, 0.5 * t, (R[..., 1, 2] + R[..., 2, 1]) * s)))
    q[..., 2] = np.where(c0, (R[..., 1, 0] - R[..., 0, 1]) * s, np.where(c1, (R[..., 0, 2] + R[..., 2, 0]) * s, np.where(c2, (R[..., 1, 2] + R[..., 2, 1]) * s, 0.5 * t)))
    return q


def aa_to_matrix(aa):
    """Rotation matrices of angle-axis vectors (..., 3) -> (..., 3, 3), as Ceres' AngleAxisToRotationMatrix computes them (its
    first-order form below theta^2 = machine epsilon included)."""
    aa = np.asarray(aa, dtype=np.float64)
    th2 = np.sum(aa * aa, axis=-1)
    big = th2 > np.finfo(np.float64).eps
    th = np.sqrt(np.where(big, th2, 1.0))
    w = aa / th[..., None]
    c, s = np.cos(th), np.sin(th)
    wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
    R = np.empty(aa.shape[:-1] + (3, 3))
    R[..., 0, 0] = c + wx * wx * (1 - c); R[..., 1, 0] = wz * s + wx * wy * (1 - c); R[..., 2, 0] = -wy * s + wx * wz * (1 - c)
    R[..., 0, 1] = wx * wy * (1 - c) - wz * s; R[..., 1, 1] = c + wy * wy * (1 - c); R[..., 2, 1] = wx * s + wy * wz * (1 - c)
    R[..., 0, 2] = wy * s + wx * wz * (1 - c); R[..., 1, 2] = -wx * s + wy * wz * (1 - c); R[..., 2, 2] = c + wz * wz * (1 - c)
    x, y, z = aa[..., 0], aa[..., 1], aa[..., 2]
    one, zero = np.ones_like(x), np.zeros_like(x)
    small = np.stack([np.stack([one, -z, y], -1), np.stack([z, one, -x], -1), np.stack([-y, x, one], -1)], -2)
    return np.where(big[..., None, None], R, small)


def make_position_graph(n_cams, n_edges, seed, outlier_frac=0.0, noise=0.0, extent=10.0, local_window=0):
    """Returns dict(n_cams, edge_i, edge_j, rel_t, rot_aa, gt_pos, is_outlier) for camera-position estimation.

    The rotations and the edge set are those make_graph(n_cams, n_edges, seed) draws (its ground-truth rotations, then make_edges from
    the same generator), so the benchmark graph of the rotation path and this one share their topology.  Positions are uniform in a cube
    of side 2 * extent; rel_t = position_2 = R_i (c_j - c_i) / |c_j - c_i|, its world direction perturbed by N(0, noise^2) per component
    and renormalised; outliers (only among the non-chain edges) get uniform random unit directions.  local_window > 0: edges only
    between cameras close in a hidden ordering (make_local_edges: a normal matrix that a sparse direct solver factorises with
    little fill-in; not the benchmark's topology)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rot_aa = 0.2 * rng.uniform(-1.0, 1.0, (n_cams, 3))
    ei, ej = make_local_edges(rng, n_cams, n_edges, local_window) if local_window else make_edges(rng, n_cams, n_edges)
    E = ei.shape[0]
    gt = extent * rng.uniform(-1.0, 1.0, (n_cams, 3))
    d = gt[ej] - gt[ei]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if noise > 0:
        d = d + noise * rng.standard_normal((E, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    is_out = np.zeros(E, dtype=bool)
    if outlier_frac > 0:
        cand = np.arange(n_cams - 1, E)
        k = int(round(outlier_frac * E))
        pick = rng.choice(cand, size=min(k, cand.size), replace=False)
        is_out[pick] = True
        u = rng.standard_normal((pick.size, 3))
        d[pick] = u / np.linalg.norm(u, axis=1, keepdims=True)
    rel_t = np.empty((E, 3))
    for b0 in range(0, E, 1 << 22):   # R_i d in blocks (the 10M-edge graph)
        sl = slice(b0, min(E, b0 + (1 << 22)))
        rel_t[sl] = np.einsum("eij,ej->ei", aa_to_matrix(rot_aa[ei[sl]]), d[sl])
    return {"n_cams": int(n_cams), "edge_i": ei, "edge_j": ej, "rel_t": rel_t, "rot_aa": rot_aa, "gt_pos": gt, "is_outlier": is_out}


def make_tracks(n_cams, n_tracks, seed, lengths=(2, 3, 4, 5, 8, 13), length_weights=None, noise_px=0.5, outlier_frac=0.0, outlier_px=(50.0, 300.0)):
    """Returns dict(n_cams, rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, gt_points, is_outlier) for track triangulation
    (include/gsfm_tracks.h): cameras on a ring of radius 9 to 12 looking at a point cloud in the cube [-2, 2]^3 with a little jitter,
    pinhole intrinsics f u v; every track is one point, its length drawn from `lengths` (with probabilities `length_weights`, uniform when
    None); the k-th observation of a track is taken by camera sigma[(a + k) mod n_cams], sigma a fixed permutation and a the track's random
    offset, so a track's cameras are distinct up to n_cams observations and repeat beyond; pixels carry N(0, noise_px^2) noise and a
    fraction outlier_frac of the observations is moved by outlier_px[0] .. outlier_px[1] pixels in a random direction.  Seeded (PCG64) and
    vectorised (10 M observations take seconds)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = rng.uniform(0.0, 2.0 * np.pi, n_cams)
    rad = rng.uniform(9.0, 12.0, n_cams)
    cam_pos = np.c_[rad * np.sin(ang), rng.uniform(-1.5, 1.5, n_cams), -rad * np.cos(ang)]
    z = 0.3 * rng.standard_normal((n_cams, 3)) - cam_pos
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)                       # world -> camera, rows x y z
    R = quat_to_matrix(aa_to_quat(0.05 * rng.standard_normal((n_cams, 3)))) @ R
    rot_aa = np.ascontiguousarray(quat_to_aa(matrix_to_quat(R)))
    intrinsics = np.c_[rng.uniform(900.0, 1500.0, n_cams), rng.integers(500, 700, n_cams).astype(np.float64),
                       rng.integers(350, 450, n_cams).astype(np.float64)]
    lengths = np.asarray(lengths, dtype=np.int64)
    length = lengths[rng.choice(lengths.size, size=n_tracks, p=length_weights)]
    track_ptr = np.concatenate([[0], np.cumsum(length)]).astype(np.uint64)
    n_obs = int(track_ptr[-1])
    gt = rng.uniform(-2.0, 2.0, (n_tracks, 3))
    sigma = rng.permutation(n_cams)
    offset = rng.integers(0, n_cams, n_tracks)
    track_of = np.repeat(np.arange(n_tracks, dtype=np.int64), length)
    place = np.arange(n_obs, dtype=np.int64) - np.repeat(track_ptr[:-1].astype(np.int64), length)
    obs_cam = sigma[(offset[track_of] + place) % n_cams].astype(np.uint32)
    Rm = aa_to_matrix(rot_aa)                                            # what a consumer of rot_aa computes
    obs_xy = np.empty((n_obs, 2))
    for b0 in range(0, n_obs, 1 << 21):
        sl = slice(b0, min(n_obs, b0 + (1 << 21)))
        c = obs_cam[sl]
        p = np.einsum("eij,ej->ei", Rm[c], gt[track_of[sl]] - cam_pos[c])
        obs_xy[sl] = intrinsics[c, :1] * p[:, :2] / p[:, 2:] + intrinsics[c, 1:]
    obs_xy += noise_px * rng.standard_normal((n_obs, 2))
    is_out = rng.random(n_obs) < outlier_frac
    k = int(is_out.sum())
    if k:
        th, r = rng.uniform(0.0, 2.0 * np.pi, k), rng.uniform(outlier_px[0], outlier_px[1], k)
        obs_xy[is_out] += np.c_[r * np.cos(th), r * np.sin(th)]
    return {"n_cams": int(n_cams), "rot_aa": rot_aa, "cam_pos": cam_pos, "intrinsics": intrinsics, "track_ptr": track_ptr, "obs_cam": obs_cam,
            "obs_xy": obs_xy, "gt_points": gt, "is_outlier": is_out}


def make_position_scene(n_cams, n_edges, n_tracks, seed, lengths=(2, 3, 4, 5, 8, 13), noise=0.0, outlier_frac=0.0, extent=10.0):
    """A position graph and feature tracks over the same ground-truth cameras (include/gsfm_posp.h): make_position_graph(n_cams, n_edges, seed,
    outlier_frac, noise, extent)'s dict plus intrinsics (N x 3: f u v), track_ptr, obs_cam, obs_xy and gt_points.  The points lie in a slab
    4 .. 6 extent in front of the cameras (whose rotations are small, so every point is in front of every camera); a track's k-th observation
    is taken by camera sigma[(a + k) mod n_cams] (make_tracks' rule: distinct cameras up to n_cams observations), its length drawn from
    `lengths`; the pixels are the ground-truth projections with R = aa_to_matrix(rot_aa), plus N(0, (noise f)^2) per coordinate."""
    g = make_position_graph(n_cams, n_edges, seed, outlier_frac=outlier_frac, noise=noise, extent=extent)
    rng = np.random.Generator(np.random.PCG64([seed, 1]))
    intrinsics = np.c_[rng.uniform(900.0, 1500.0, n_cams), rng.integers(500, 700, n_cams).astype(np.float64),
                       rng.integers(350, 450, n_cams).astype(np.float64)]
    lengths = np.asarray(lengths, dtype=np.int64)
    length = lengths[rng.choice(lengths.size, size=n_tracks)]
    track_ptr = np.concatenate([[0], np.cumsum(length)]).astype(np.uint64)
    n_obs = int(track_ptr[-1])
    gt = np.c_[extent * rng.uniform(-1.0, 1.0, (n_tracks, 2)), extent * rng.uniform(4.0, 6.0, n_tracks)]
    sigma = rng.permutation(n_cams)
    offset = rng.integers(0, n_cams, n_tracks)
    track_of = np.repeat(np.arange(n_tracks, dtype=np.int64), length)
    place = np.arange(n_obs, dtype=np.int64) - np.repeat(track_ptr[:-1].astype(np.int64), length)
    obs_cam = sigma[(offset[track_of] + place) % n_cams].astype(np.uint32)
    p = np.einsum("eij,ej->ei", aa_to_matrix(g["rot_aa"])[obs_cam], gt[track_of] - g["gt_pos"][obs_cam])
    obs_xy = intrinsics[obs_cam, :1] * p[:, :2] / p[:, 2:] + intrinsics[obs_cam, 1:]
    if noise > 0:
        obs_xy = obs_xy + noise * intrinsics[obs_cam, :1] * rng.standard_normal((n_obs, 2))
    g.update(intrinsics=intrinsics, track_ptr=track_ptr, obs_cam=obs_cam, obs_xy=np.ascontiguousarray(obs_xy), gt_points=gt)
    return g


def gauge_normalize(pos, fixed_cam):
    """Positions with translation and scale removed: subtract the fixed camera, divide by the RMS distance from it."""
    p = np.asarray(pos, dtype=np.float64) - np.asarray(pos, dtype=np.float64)[fixed_cam]
    rms = np.sqrt(np.mean(np.sum(p * p, axis=1)))
    return p / rms if rms > 0 else p
