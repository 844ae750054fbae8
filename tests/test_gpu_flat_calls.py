"""-m gpu: the one-shot calls on the scratch owner of csrc/flat_call.hpp return the same bytes call after call.  gsfm_cov_estimate runs
on a private stream like the others: three calls in one process, with a RotationProblem alive and solving on its own stream in between,
must agree byte for byte.  gsfm_rot_init_spanning_tree and gsfm_rot_edge_sq_norms: two calls each on small graphs."""
import math

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import covariance as cv
from globalsfmpy_amd.solver import RotationProblem, edge_sq_norms, orientations_from_maximum_spanning_tree as mst_init

import cov_hp_reference as CR

pytestmark = pytest.mark.gpu


def test_cov_estimate_repeats_beside_a_live_problem():
    """6 edges: one without matches (status 1), one with two matches -- fewer than the five unknowns need (status 2) -- and four ordinary."""
    m, K, r, t = CR.make_edge(71, 40)
    edges = [CR.make_edge(72, 64), (np.zeros((0, 4)), K, r, t), CR.make_edge(73, 129), (m[:2], K, r, t), (m, K, r, t), CR.make_edge(74, 65)]
    b = CR.batch(edges)
    g = synth.make_graph(n_cams=60, n_edges=400, seed=7, outlier_frac=0.1)
    prob = RotationProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], _abi.ANGLE_AXIS_COVARIANCE, cov6=g["cov6"])
    outs = []
    for _ in range(3):
        outs.append(cv.estimate_rotation_covariances(b["match_ptr"], b["matches"], b["intrinsics"], b["rot"], b["trans"], max_iterations=500))
        _, summary = prob.solve(g["init_aa"])
        assert math.isfinite(summary["final_cost"])
    prob.close()
    np.testing.assert_array_equal(outs[0]["status"], [0, 1, 0, 2, 0, 0])
    for o in outs:
        assert math.isfinite(o["kernel_ms"]) and o["kernel_ms"] > 0.0
        for key in ("cov", "rotation", "translation", "status", "iterations"):
            assert o[key].tobytes() == outs[0][key].tobytes(), key


def test_spanning_tree_repeats_on_16_cameras():
    # the components graph of test_gpu_spanning_tree.py (cameras 0 .. 15): Y = {1, 2, 9, 10, 15} wins
    ei = np.array([3, 4, 7, 8, 1, 2, 9, 10, 0, 2], dtype=np.uint32)
    ej = np.array([4, 7, 8, 11, 2, 9, 10, 15, 5, 15], dtype=np.uint32)
    rel = 0.2 * np.random.default_rng(3).standard_normal((ei.size, 3))
    w = np.array([5, 5, 5, 5, 1, 1, 1, 1, 9, 0], dtype=np.int32)
    a, b = mst_init(16, ei, ej, rel, w), mst_init(16, ei, ej, rel, w)
    assert a["root"] == 1 and a["n_tree_cams"] == 5
    assert a["rot_aa"].tobytes() == b["rot_aa"].tobytes()
    assert a["parent_edge"].tobytes() == b["parent_edge"].tobytes()
    assert (a["root"], a["n_tree_cams"], a["depth"]) == (b["root"], b["n_tree_cams"], b["depth"])
    assert math.isfinite(a["kernel_ms"]) and a["kernel_ms"] > 0.0


@pytest.mark.parametrize("with_cov", [False, True])
@pytest.mark.parametrize("n_cams,n_edges", [(2, 1), (5, 7)])
def test_edge_sq_norms_repeats(n_cams, n_edges, with_cov):
    rng = np.random.default_rng(100 * n_cams + n_edges)
    pairs = np.array([(i, j) for i in range(n_cams) for j in range(i + 1, n_cams)], dtype=np.uint32)[:n_edges]
    rel = 0.3 * rng.standard_normal((n_edges, 3))
    rot = 0.3 * rng.standard_normal((n_cams, 3))
    cov6 = None
    if with_cov:
        cov6 = np.zeros((n_edges, 6))
        cov6[:, :3] = rng.uniform(1e-4, 1e-2, (n_edges, 3))   # C00 C11 C22; no off-diagonal terms
    a = edge_sq_norms(n_cams, pairs[:, 0], pairs[:, 1], rel, rot, cov6=cov6, max_sq_norm=1.0)
    b = edge_sq_norms(n_cams, pairs[:, 0], pairs[:, 1], rel, rot, cov6=cov6, max_sq_norm=1.0)
    assert np.isfinite(a["s"]).all() and a["n_kept"] == int(a["keep"].sum())
    assert a["s"].tobytes() == b["s"].tobytes() and a["keep"].tobytes() == b["keep"].tobytes() and a["n_kept"] == b["n_kept"]
