"""The host layer of the robust L1 + IRLS rotation estimator: theia::RobustRotationEstimator through the module on view-graph maps equals
the flat-array call, a pair added twice is an edge listed twice, and GlobalReconstructionEstimator.EstimateGlobalRotationsFromOptions()
runs the estimator that the YAML key global_rotation_estimator names."""
import os
import sys

import numpy as np
import pytest

from globalsfmpy_amd import solver, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives, as the reference's scripts append ../build

pytestmark = pytest.mark.gpu


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


@pytest.fixture(scope="module")
def graph():
    g = synth.make_graph(n_cams=40, n_edges=240, seed=61, outlier_frac=0.2)
    g["ids"] = 5 + 3 * np.arange(40)   # view ids that are not the camera indices
    return g


def orientation_map(sfm, ids, rot):
    o = sfm.MapViewIdVector3d()
    for v, r in zip(ids, rot):
        o[int(v)] = np.asarray(r, dtype=np.float64)
    return o


def view_graph(sfm, g):
    vg = sfm.ViewGraph()
    for i, j, r in zip(g["edge_i"], g["edge_j"], g["rel_aa"]):
        info = sfm.TwoViewInfo()
        info.rotation_2 = r
        vg.AddEdge(int(g["ids"][i]), int(g["ids"][j]), info)
    return vg


def sorted_edges(g):
    """the graph's edges in ViewIdPair order, as camera indices (ids ascend with the index)"""
    order = np.lexsort((g["edge_j"], g["edge_i"]))
    return g["edge_i"][order], g["edge_j"][order], g["rel_aa"][order]


def as_array(o, ids):
    return np.array([o[int(v)] for v in ids])


def test_estimator_on_maps_equals_the_flat_call(graph):
    sfm = _sfm()
    vg = view_graph(sfm, graph)
    o = orientation_map(sfm, graph["ids"], graph["init_aa"])
    est = sfm.RobustRotationEstimator(sfm.RobustRotationEstimatorOptions())
    assert est.EstimateRotations(vg.GetAllEdges(), o), est.LastError()
    fixed = int(np.flatnonzero(graph["ids"] == est.FixedView())[0])
    ei, ej, rel = sorted_edges(graph)
    rot, summary = solver.estimate_rotations_robust_l1l2(40, ei, ej, rel, graph["init_aa"], fixed)
    assert as_array(o, graph["ids"]).tobytes() == rot.tobytes()
    s = est.LastSummary()
    assert s["num_admm_iterations"] == summary["num_admm_iterations"] and s["num_irls_iterations"] == summary["num_irls_iterations"]
    assert s["num_cg_iterations"] == summary["num_cg_iterations"] and s["num_edges_used"] == 240
    assert np.all(rot[fixed] == graph["init_aa"][fixed])


def test_a_pair_added_twice_is_an_edge_listed_twice(graph):
    sfm = _sfm()
    ei, ej, rel = sorted_edges(graph)
    rng = np.random.default_rng(3)
    again = rng.choice(240, 20, replace=False)
    rel2 = rel[again] + np.radians(1.0) * rng.standard_normal((20, 3))
    ei2, ej2, rel_all = np.concatenate([ei, ei[again]]), np.concatenate([ej, ej[again]]), np.concatenate([rel, rel2])
    o = orientation_map(sfm, graph["ids"], graph["init_aa"])
    est = sfm.RobustRotationEstimator()
    for i, j, r in zip(ei2, ej2, rel_all):
        est.AddRelativeRotationConstraint((int(graph["ids"][i]), int(graph["ids"][j])), r)
    assert est.EstimateRotations(o), est.LastError()
    fixed = int(np.flatnonzero(graph["ids"] == est.FixedView())[0])
    rot, summary = solver.estimate_rotations_robust_l1l2(40, ei2, ej2, rel_all, graph["init_aa"], fixed)
    assert as_array(o, graph["ids"]).tobytes() == rot.tobytes()
    assert est.LastSummary()["num_edges_used"] == 260
    once, _ = solver.estimate_rotations_robust_l1l2(40, ei, ej, rel, graph["init_aa"], fixed)
    assert np.abs(once - rot).max() > 1e-6   # the second listings count


def test_a_constraint_on_an_unknown_view_is_refused(graph):
    sfm = _sfm()
    o = orientation_map(sfm, graph["ids"][:3], graph["init_aa"][:3])
    est = sfm.RobustRotationEstimator()
    est.AddRelativeRotationConstraint((5, 8), np.zeros(3))
    est.AddRelativeRotationConstraint((5, 999), np.zeros(3))
    assert not est.EstimateRotations(o)
    assert "constraint 1 names a view without an initial orientation" in est.LastError()


def estimator_from_yaml(sfm, tmp_path, text, g):
    path = tmp_path / "flags.yaml"
    path.write_text(text)
    options = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(path), options)
    vg, rec = view_graph(sfm, g), sfm.Reconstruction()
    est = sfm.GlobalReconstructionEstimator(options.reconstruction_estimator_options)
    assert est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    return est, vg, options


def test_the_yaml_key_selects_the_robust_estimator(graph, tmp_path):
    sfm = _sfm()
    est, vg, options = estimator_from_yaml(sfm, tmp_path, "num_threads: 1\nglobal_rotation_estimator: ROBUST_L1L2\n", graph)
    assert options.reconstruction_estimator_options.global_rotation_estimator_type == sfm.GlobalRotationEstimatorType.ROBUST_L1L2
    assert est.EstimateGlobalRotationsFromOptions(), est.LastError()
    s = est.LastRobustRotationSummary()
    assert s["num_l1_iterations"] >= 1 and len(s["num_admm_iterations"]) == s["num_l1_iterations"] and s["num_irls_iterations"] >= 1
    assert s["num_edges_used"] == 240 and s["nonfinite"] == 0
    # the same as the estimator itself from the spanning-tree start
    start = sfm.MapViewIdVector3d()
    assert sfm.OrientationsFromMaximumSpanningTree(vg, start)
    direct = sfm.RobustRotationEstimator()
    assert direct.EstimateRotations(vg.GetAllEdges(), start)
    assert as_array(est.orientations, graph["ids"]).tobytes() == as_array(start, graph["ids"]).tobytes()
    err = synth.angular_distance(synth.align_rotations(as_array(est.orientations, graph["ids"]), graph["gt_aa"]), graph["gt_aa"])
    assert np.degrees(np.median(err)) < 2.0


def test_nonlinear_is_the_default_and_runs_the_nonlinear_estimator(graph, tmp_path):
    sfm = _sfm()
    assert sfm.ReconstructionEstimatorOptions().global_rotation_estimator_type == sfm.GlobalRotationEstimatorType.NONLINEAR
    for text in ("num_threads: 1\n", "num_threads: 1\nglobal_rotation_estimator: NONLINEAR\n"):
        est, vg, options = estimator_from_yaml(sfm, tmp_path, text, graph)
        assert options.reconstruction_estimator_options.global_rotation_estimator_type == sfm.GlobalRotationEstimatorType.NONLINEAR
        assert est.EstimateGlobalRotationsFromOptions(), est.LastError()
        start = sfm.MapViewIdVector3d()
        assert sfm.OrientationsFromMaximumSpanningTree(vg, start)
        direct = sfm.NonlinearRotationEstimator()
        assert direct.EstimateRotations(vg.GetAllEdges(), start)
        assert as_array(est.orientations, graph["ids"]).tobytes() == as_array(start, graph["ids"]).tobytes()
        assert est.LastSummary()["num_iterations"] == direct.LastSummary()["num_iterations"] > 0
        assert est.LastRobustRotationSummary()["num_l1_iterations"] == 0


def test_linear_returns_false_and_says_why(graph, tmp_path):
    sfm = _sfm()
    est, vg, options = estimator_from_yaml(sfm, tmp_path, "global_rotation_estimator: LINEAR\n", graph)
    assert options.reconstruction_estimator_options.global_rotation_estimator_type == sfm.GlobalRotationEstimatorType.LINEAR
    assert est.EstimateGlobalRotationsFromOptions() is False
    assert "LINEAR" in est.LastError() and "not built" in est.LastError()
    with pytest.raises(ValueError, match="no such estimator 'L1'"):
        estimator_from_yaml(sfm, tmp_path, "global_rotation_estimator: L1\n", graph)
