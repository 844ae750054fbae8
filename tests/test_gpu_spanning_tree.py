"""-m gpu: gsfm_rot_init_spanning_tree (theia's OrientationsFromMaximumSpanningTree on the device) against scipy's minimum spanning
tree, a union-find Kruskal, the host implementation of the C++ layer, and noise-free graphs."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))

from globalsfmpy_amd import _abi, synth  # noqa: E402
from globalsfmpy_amd import loss_functions as LF  # noqa: E402
from globalsfmpy_amd.solver import RotationProblem, SolverError, edge_sq_norms, orientations_from_maximum_spanning_tree as mst_init  # noqa: E402

pytestmark = pytest.mark.gpu


def _random_pairs(rng, n, m):
    """m distinct unordered pairs i < j, in random order."""
    keys = np.empty(0, dtype=np.int64)
    while keys.size < m:
        a, b = rng.integers(0, n, 2 * m), rng.integers(0, n, 2 * m)
        ok = a != b
        keys = np.unique(np.concatenate([keys, np.minimum(a, b)[ok] * n + np.maximum(a, b)[ok]]))
    keys = rng.permutation(keys)[:m]
    return (keys // n).astype(np.uint32), (keys % n).astype(np.uint32)


def _tree_edges(out):
    pe = out["parent_edge"]
    return np.sort(pe[pe >= 0])


def _component(n, ei, ej, root):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    _, lab = connected_components(sp.coo_matrix((np.ones(ei.size), (ei, ej)), shape=(n, n)), directed=False)
    return lab == lab[root]


def _scipy_tree(n, ei, ej, w):
    """Edge indices of scipy's minimum spanning tree on the distinct keys -(w E + (E - e)): the maximum tree under (w desc, e asc)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    E = ei.size
    key = -(w.astype(np.float64) * E + (E - np.arange(E, dtype=np.float64)))
    t = minimum_spanning_tree(sp.coo_matrix((key, (ei.astype(np.int64), ej.astype(np.int64))), shape=(n, n)).tocsr()).tocoo()
    v = np.rint(-t.data).astype(np.int64)   # w E + (E - e), E - e in [1, E]
    return np.sort(E - (v - (v - 1) // E * E))


def _kruskal(n, ei, ej, w):
    p = list(range(n))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x
    out = []
    for e in sorted(range(ei.size), key=lambda e: (-int(w[e]), e)):
        a, b = find(int(ei[e])), find(int(ej[e]))
        if a != b:
            p[a] = b
            out.append(e)
    return np.array(sorted(out), dtype=np.int64)


def _check_composition(out, ei, ej, rel, tol):
    """Every tree edge's relative rotation reproduced: angle(R_j R_i^T, R_ij)."""
    e = _tree_edges(out)
    q = synth.aa_to_quat(out["rot_aa"])
    got = synth.quat_mul(q[ej[e]], synth.quat_conj(q[ei[e]]))
    ang = synth.angular_distance(synth.quat_to_aa(got), rel[e])
    assert ang.max() <= tol, ang.max()
    return ang.max()


@pytest.mark.parametrize("n,m", [(2000, 40000), (20000, 2000000)])
def test_tie_break_matches_scipy_on_distinct_keys(n, m):
    rng = np.random.default_rng(n)
    ei, ej = _random_pairs(rng, n, m)
    w = rng.integers(0, 4, m).astype(np.int32)   # four weights: most comparisons tie
    rel = 0.3 * rng.standard_normal((m, 3))
    out = mst_init(n, ei, ej, rel, w)
    want = _scipy_tree(n, ei, ej, w)
    comp = _component(n, ei, ej, out["root"])
    want = want[comp[ei[want]]]
    np.testing.assert_array_equal(_tree_edges(out), want)
    assert out["n_tree_cams"] == comp.sum() and out["root"] == int(np.flatnonzero(comp)[0])
    _check_composition(out, ei, ej, rel, 1e-12)


def test_duplicate_pairs_break_ties_by_index_like_kruskal():
    rng = np.random.default_rng(5)
    n = 300
    ei, ej = _random_pairs(rng, n, 2000)
    dup = rng.integers(0, ei.size, 800)
    flip = rng.random(dup.size) < 0.5
    ei, ej = np.concatenate([ei, np.where(flip, ej[dup], ei[dup])]), np.concatenate([ej, np.where(flip, ei[dup], ej[dup])])
    perm = rng.permutation(ei.size)
    ei, ej = ei[perm], ej[perm]
    w = rng.integers(0, 3, ei.size).astype(np.int32)
    rel = 0.3 * rng.standard_normal((ei.size, 3))
    out = mst_init(n, ei, ej, rel, w)
    np.testing.assert_array_equal(_tree_edges(out), _kruskal(n, ei, ej, w))
    _check_composition(out, ei, ej, rel, 1e-12)


def _host_vs_device(sfm, vg, ids):
    host, dev = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    assert sfm.OrientationsFromMaximumSpanningTree(vg, host)
    assert sfm.OrientationsFromMaximumSpanningTreeOnDevice(vg, dev)
    hk, dk = sorted(int(k) for k in host.keys()), sorted(int(k) for k in dev.keys())
    assert hk == dk
    a = np.array([host[k] for k in hk])
    b = np.array([dev[k] for k in hk])
    d = synth.angular_distance(a, b)
    assert d.max() <= 1e-10, d.max()
    return d.max()


def test_device_matches_host_on_madrid_and_on_sparse_view_ids(golden_dir):
    sfm = pytest.importorskip("GlobalSfMpy")
    m = np.load(os.path.join(golden_dir, "madrid_graph.npz"))
    vg = sfm.ViewGraph()
    for a_, b_, r_ in zip(m["edge_a"], m["edge_b"], m["rel_aa"]):   # every weight 1: the tree is pure tie-break
        info = sfm.TwoViewInfo()
        info.rotation_2 = r_
        info.num_verified_matches = 1
        vg.AddEdge(int(a_), int(b_), info)
    _host_vs_device(sfm, vg, m["view_ids"])
    rng = np.random.default_rng(80)
    ids = np.sort(rng.choice(10 ** 6, 80, replace=False))
    ei, ej = _random_pairs(rng, 80, 400)
    vg = sfm.ViewGraph()
    for i, j in zip(ei, ej):
        info = sfm.TwoViewInfo()
        info.rotation_2 = rng.standard_normal(3)
        info.num_verified_matches = int(rng.integers(0, 4))
        vg.AddEdge(int(ids[j]), int(ids[i]), info)   # (either order: the key is normalised)
    _host_vs_device(sfm, vg, ids)


def test_noise_free_graph_reproduces_every_tree_edge():
    g = synth.make_graph(3000, 30000, seed=11, noise=False, full_so3=True)
    w = np.random.default_rng(1).integers(0, 100, g["edge_i"].size).astype(np.int32)
    out = mst_init(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], w)
    assert out["n_tree_cams"] == 3000 and out["root"] == 0
    _check_composition(out, g["edge_i"], g["edge_j"], g["rel_aa"], 1e-12)
    err = synth.angular_distance(synth.align_rotations(out["rot_aa"], g["gt_aa"]), g["gt_aa"])
    assert err.max() <= 1e-10


def test_components_largest_with_ties_to_the_smallest_camera():
    # X = {3, 4, 7, 8, 11} and Y = {1, 2, 9, 10, 15}: five cameras each, Y holds camera 1 and wins; Z = {0, 5}; the rest isolated
    ei = np.array([3, 4, 7, 8, 1, 2, 9, 10, 0, 2], dtype=np.uint32)
    ej = np.array([4, 7, 8, 11, 2, 9, 10, 15, 5, 15], dtype=np.uint32)
    rel = 0.2 * np.random.default_rng(3).standard_normal((ei.size, 3))
    out = mst_init(20, ei, ej, rel, np.array([5, 5, 5, 5, 1, 1, 1, 1, 9, 0], dtype=np.int32))
    assert out["root"] == 1 and out["n_tree_cams"] == 5
    inside = np.zeros(20, dtype=bool)
    inside[[1, 2, 9, 10, 15]] = True
    assert (out["parent_edge"][~inside] == -1).all() and not out["rot_aa"][~inside].any()
    assert out["parent_edge"][1] == -1 and not out["rot_aa"][1].any()
    np.testing.assert_array_equal(_tree_edges(out), [4, 5, 6, 7])   # edge 9 (2, 15) weighs 0 and closes the cycle 2-9-10-15
    _check_composition(out, ei, ej, rel, 1e-12)


def test_no_edges_is_empty():
    with pytest.raises(SolverError, match="status 4"):
        mst_init(6, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3)))


def test_chain_and_star_depths():
    n = 50000
    rng = np.random.default_rng(9)
    gt = synth.quat_to_aa(synth.random_unit_quat(rng, n))
    q = synth.aa_to_quat(gt)
    k = np.arange(n - 1)
    perm = rng.permutation(n - 1)                       # chain edges in random order, random orientation
    up = rng.random(n - 1) < 0.5
    ei = np.where(up, k, k + 1)[perm].astype(np.uint32)
    ej = np.where(up, k + 1, k)[perm].astype(np.uint32)
    rel = synth.quat_to_aa(synth.quat_mul(q[ej], synth.quat_conj(q[ei])))
    t0 = time.perf_counter()
    out = mst_init(n, ei, ej, rel)
    dt = time.perf_counter() - t0
    print("chain of %d cameras: depth %d, %.1f ms wall, %.2f ms kernels" % (n, out["depth"], 1e3 * dt, out["kernel_ms"]))
    assert out["depth"] == n - 1 and out["root"] == 0 and out["n_tree_cams"] == n
    want = synth.quat_to_aa(synth.quat_mul(q, synth.quat_conj(q[:1])))   # R_k R_0^T
    assert synth.angular_distance(out["rot_aa"], want).max() <= 1e-9
    _check_composition(out, ei, ej, rel, 1e-12)
    ei = np.zeros(n - 1, dtype=np.uint32)
    ej = np.arange(1, n, dtype=np.uint32)
    rel = 0.5 * rng.standard_normal((n - 1, 3))
    out = mst_init(n, ej, ei, rel)                      # (k, 0): R_0 = R_k0 R_k, so R_k = R_k0^T
    assert out["depth"] == 1 and out["root"] == 0
    np.testing.assert_array_equal(out["parent_edge"][1:], np.arange(n - 1))
    assert synth.angular_distance(out["rot_aa"][1:], -rel).max() <= 1e-12


def test_two_calls_return_the_same_bytes():
    rng = np.random.default_rng(20)
    ei, ej = _random_pairs(rng, 20000, 2000000)
    w = rng.integers(0, 4, ei.size).astype(np.int32)
    rel = rng.standard_normal((ei.size, 3))
    a, b = mst_init(20000, ei, ej, rel, w), mst_init(20000, ei, ej, rel, w)
    assert a["rot_aa"].tobytes() == b["rot_aa"].tobytes()
    assert a["parent_edge"].tobytes() == b["parent_edge"].tobytes()
    assert (a["root"], a["n_tree_cams"], a["depth"]) == (b["root"], b["n_tree_cams"], b["depth"])


def test_c5_tree_start():
    g = synth.make_graph(100_000, 10_000_000, seed=2023, outlier_frac=0.3)
    init_ref, matches = synth.spanning_tree_init(g, 2023)
    ei, ej = g["edge_i"], g["edge_j"]
    out = mst_init(g["n_cams"], ei, ej, g["rel_aa"], matches.astype(np.int32))
    assert out["n_tree_cams"] == g["n_cams"]
    e = _tree_edges(out)
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    t = minimum_spanning_tree(sp.coo_matrix((-matches.astype(np.float64), (ei.astype(np.int64), ej.astype(np.int64))), shape=(g["n_cams"],) * 2).tocsr())
    assert int(matches[e].sum()) == int(round(-t.sum()))
    s = edge_sq_norms(g["n_cams"], ei[e], ej[e], g["rel_aa"][e], out["rot_aa"])["s"]
    assert np.sqrt(s.max()) <= 1e-12
    prob = RotationProblem(g["n_cams"], ei, ej, g["rel_aa"], _abi.ANGLE_AXIS_COVARIANCE, cov6=g["cov6"])
    prob.set_loss(LF.MAGSACWeightBasedLoss(0.02))
    _, sd = prob.solve(out["rot_aa"])
    _, sr = prob.solve(init_ref)
    print("C5 from the device tree: %d LM iterations, %s; from synth.spanning_tree_init: %d, %s"
          % (sd["num_iterations"], sd["termination_name"], sr["num_iterations"], sr["termination_name"]))
    assert sd["termination_name"] == sr["termination_name"] and sd["termination_name"] not in ("NO_CONVERGENCE", "FAILURE")
