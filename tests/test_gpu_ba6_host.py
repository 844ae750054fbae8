"""-m gpu: the host layer of the full bundle adjustment on the synthetic 1DSfM dataset of test_gpu_ba_host.py: after EstimateStructure and
SetUnderconstrainedAsUnestimated, GlobalReconstructionEstimator.BundleAdjustment() stores exactly what solver.bundle_adjust returns on the
flattened arrays -- orientations and positions of the estimated views, points of the estimated tracks -- lowers the cost and leaves the
unestimated view and tracks untouched."""
import numpy as np
import pytest

from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import bundle_adjust

from test_gpu_ba_host import UNESTIMATED_VIEW, _pipeline_up_to_structure, dataset, scene  # noqa: F401  (the fixtures and the pipeline of the fixed-orientation test)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float64)).view(np.uint64)


def test_host_call_stores_what_the_flat_call_returns(dataset, scene):  # noqa: F811
    sfm, est, rec = _pipeline_up_to_structure(dataset, scene)
    T = rec.NumTracks()
    sfm.SetUnderconstrainedAsUnestimated(rec)
    flat = rec.FlattenedTracks()
    pt_est = np.array([rec.TrackIsEstimated(t) for t in range(T)], np.uint8)
    pts0 = np.array([rec.TrackPoint(t) for t in range(T)])
    rot_before = {v: np.array(w) for v, w in rec.EstimatedOrientations().items()}
    pos_before = {v: np.array(p) for v, p in rec.EstimatedPositions().items()}
    assert pt_est.sum() >= 30 and flat["cam_estimated"].sum() == 11 and UNESTIMATED_VIEW not in pos_before
    w1, c1, p1, s = bundle_adjust(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"], pts0,
                                  flat["cam_estimated"], pt_est, loss=LF.HuberLoss(10.0))
    assert est.BundleAdjustment() is True
    st = est.LastBundleAdjustmentSummary()
    print("BundleAdjustment: %s" % st)
    assert st["ran"] and st["usable"] and st["max_num_iterations"] == 100
    assert (st["termination"], st["num_iterations"], st["num_cg_iterations"]) == (s["termination"], s["num_iterations"], s["num_cg_iterations"])
    assert st["initial_cost"] == s["initial_cost"] and st["final_cost"] == s["final_cost"] and st["final_cost"] < st["initial_cost"]
    assert st["num_cameras"] == 11 and st["num_points"] == pt_est.sum()
    rot_after, pos_after = rec.EstimatedOrientations(), rec.EstimatedPositions()
    assert sorted(rot_after.keys()) == sorted(rot_before.keys()) and sorted(pos_after.keys()) == sorted(pos_before.keys())
    for c, v in enumerate(flat["views"]):
        if flat["cam_estimated"][c]:
            assert np.array_equal(_bits(rot_after[int(v)]), _bits(w1[c])) and np.array_equal(_bits(pos_after[int(v)]), _bits(c1[c])), v
    for t in range(T):
        assert np.array_equal(_bits(rec.TrackPoint(t)), _bits(p1[t])), t
        assert rec.TrackIsEstimated(t) == bool(pt_est[t])
        if not pt_est[t]:
            assert np.array_equal(_bits(rec.TrackPoint(t)), _bits(pts0[t])), t
    # orientations and positions both moved
    assert any(not np.array_equal(np.array(rot_after[v]), rot_before[v]) for v in rot_before)
    assert any(not np.array_equal(np.array(pos_after[v]), pos_before[v]) for v in pos_before)
    # the unestimated view is still unestimated
    assert UNESTIMATED_VIEW not in rot_after and UNESTIMATED_VIEW not in pos_after


def test_iteration_rule_unknown_loss_and_a_dataset_without_tracks(dataset, scene, tmp_path):  # noqa: F811
    sfm, est, rec = _pipeline_up_to_structure(dataset, scene)
    est.options.min_cameras_for_iterative_solver = 12    # the reconstruction has 12 views: 1.5 x the iterations
    assert est.BundleAdjustment() and est.LastBundleAdjustmentSummary()["max_num_iterations"] == 150
    est.options.bundle_adjustment_loss_function_type = "CAUCHY"
    with pytest.raises(RuntimeError, match="BundleAdjustment: no loss CAUCHY"):
        est.BundleAdjustment()
    import os
    import shutil
    bare = tmp_path / "bare"
    bare.mkdir()
    for name in ("EGs.txt", "cc.txt"):
        shutil.copy(os.path.join(dataset, name), str(bare / name))
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(str(bare), rec, vg, cov)
    est = sfm.GlobalReconstructionEstimator(sfm.ReconstructionEstimatorOptions())
    est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    assert est.BundleAdjustment() is True and est.LastBundleAdjustmentSummary()["ran"] is False
