"""Plain numpy restatement of the relative-translation filter as include/gsfm_pos.h defines it (gsfm_pos_filter_relative_translations):
Theia's FilterViewPairsFromRelativeTranslation with integer arc weights, all sources removed per pass and the smallest camera index
among equal scores.  From the projections on everything is integer arithmetic and one fixed-order fp64 sum, so the device must agree
with `filter_from_projections` bit for bit when it is given the device's own projections."""
import numpy as np

from globalsfmpy_amd import synth

TWO32 = 1 << 32


def world_directions(edge_i, rel_t, rot_aa):
    """d_e = R(aa_i)^T t_e"""
    R = synth.aa_to_matrix(np.asarray(rot_aa, dtype=np.float64)[np.asarray(edge_i, dtype=np.int64)])
    return np.einsum("eji,ej->ei", R, np.asarray(rel_t, dtype=np.float64))


def mean_variance(d):
    E = d.shape[0]
    mean = d.sum(axis=0) / E
    var = ((d - mean) ** 2).sum(axis=0) / (E - 1) if E > 1 else np.zeros(3)
    return mean, var


def make_axes(mean, var, n_axes, seed):
    """axis_k = normalise(mean + var o z_k): the variance in the place of a standard deviation, as the reference has it.  numpy's PCG64
    normals: neither the reference's axes nor the library's."""
    z = np.random.Generator(np.random.PCG64(seed)).standard_normal((n_axes, 3))
    a = mean + var * z
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def arc_weights(p):
    """q = floor(|p| 2^32 + 0.5) as int64"""
    return np.floor(np.abs(p) * float(TWO32) + 0.5).astype(np.int64)


def build_rows(n_cams, edge_i, edge_j):
    """per-camera rows of directed entries: (row_ptr, neighbour, edge, side) with side 1 = the row is the edge's second camera"""
    ei, ej = np.asarray(edge_i, dtype=np.int64), np.asarray(edge_j, dtype=np.int64)
    E = ei.shape[0]
    row = np.concatenate([ei, ej])
    nbr = np.concatenate([ej, ei])
    edge = np.concatenate([np.arange(E), np.arange(E)])
    side = np.concatenate([np.zeros(E, dtype=bool), np.ones(E, dtype=bool)])
    order = np.argsort(row, kind="stable")
    row_ptr = np.zeros(n_cams + 1, dtype=np.int64)
    np.add.at(row_ptr, row + 1, 1)
    return np.cumsum(row_ptr), nbr[order], edge[order], side[order]


def order_passes(n_cams, rows, p):
    """The ordering under one projection p (E values).  Returns (pass number per camera, -1 for a camera without an edge; number of
    passes; number of score picks)."""
    row_ptr, nbr, edge, side = rows
    q_e = arc_weights(p)
    q = q_e[edge]
    out = (p[edge] > 0) != side          # the entry's arc leaves the row's camera
    deg = np.diff(row_ptr)
    row_of = np.repeat(np.arange(n_cams), deg)
    qin = np.zeros(n_cams, dtype=np.int64)
    qout = np.zeros(n_cams, dtype=np.int64)
    indeg = np.zeros(n_cams, dtype=np.int64)
    np.add.at(qout, row_of[out], q[out])
    np.add.at(qin, row_of[~out], q[~out])
    np.add.at(indeg, row_of[~out], 1)
    live = deg > 0
    passes = np.full(n_cams, -1, dtype=np.int64)
    n_live = int(live.sum())
    sources = np.flatnonzero(live & (indeg == 0))
    pass_no = picks = 0
    while n_live > 0:
        if sources.size:
            remove = sources
        else:
            score = np.where(live, (qout + TWO32).astype(np.float64) / (qin + TWO32).astype(np.float64), -1.0)
            remove = np.array([int(np.argmax(score))])   # the first maximum: the smallest index among equal scores
            picks += 1
        passes[remove] = pass_no
        live[remove] = False
        n_live -= remove.size
        touched = []
        for u in remove:
            sl = slice(row_ptr[u], row_ptr[u + 1])
            m, qq, oo = nbr[sl], q[sl], out[sl]
            ok = live[m]
            mo, mi = m[ok & oo], m[ok & ~oo]
            np.subtract.at(qin, mo, qq[ok & oo])
            np.subtract.at(indeg, mo, 1)
            np.subtract.at(qout, mi, qq[ok & ~oo])
            touched.append(mo)
        touched = np.unique(np.concatenate(touched))
        sources = touched[live[touched] & (indeg[touched] == 0)]
        pass_no += 1
    return passes, pass_no, picks


def inconsistent_edges(edge_i, edge_j, p, passes):
    """the arc's tail was removed in a later pass than its head"""
    pi, pj = passes[np.asarray(edge_i, dtype=np.int64)], passes[np.asarray(edge_j, dtype=np.int64)]
    return np.where(p > 0, pi > pj, pj > pi)


def filter_from_projections(n_cams, edge_i, edge_j, proj, tolerance):
    """Steps 5 to 8 on given projections (E x n_axes).  Returns dict(bad_weight, keep, passes (n_axes x n_cams), num_passes, num_picks,
    inconsistent (E x n_axes))."""
    proj = np.asarray(proj, dtype=np.float64)
    E, K = proj.shape
    rows = build_rows(n_cams, edge_i, edge_j)
    bad = np.zeros(E)
    passes = np.empty((K, n_cams), dtype=np.int64)
    n_pass, n_pick = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    inc = np.zeros((E, K), dtype=bool)
    for k in range(K):
        p = np.ascontiguousarray(proj[:, k])
        passes[k], n_pass[k], n_pick[k] = order_passes(n_cams, rows, p)
        inc[:, k] = inconsistent_edges(edge_i, edge_j, p, passes[k])
        bad = bad + np.where(inc[:, k], np.abs(p), 0.0)
    keep = ~(bad > tolerance * K)
    return {"bad_weight": bad, "keep": keep, "passes": passes, "num_passes": n_pass, "num_picks": n_pick, "inconsistent": inc}


def filter_relative_translations(n_cams, edge_i, edge_j, rel_t, rot_aa, num_iterations=48, tolerance=0.1, seed=1, axes=None):
    """All eight steps, with numpy's axes when none are given."""
    d = world_directions(edge_i, rel_t, rot_aa)
    mean, var = mean_variance(d)
    if axes is None:
        axes = make_axes(mean, var, num_iterations, seed)
    axes = np.asarray(axes, dtype=np.float64).reshape(-1, 3)
    proj = d[:, 0:1] * axes[:, 0] + d[:, 1:2] * axes[:, 1] + d[:, 2:3] * axes[:, 2]
    out = filter_from_projections(n_cams, edge_i, edge_j, proj, tolerance)
    out.update(mean=mean, variance=var, axes=axes, projections=proj, directions=d)
    return out
