"""-m gpu: intrinsics_to_optimize through the host layer, on a synthetic 1DSfM dataset (test_gpu_ba_host.py's scene) whose list.txt focal
lengths are off from the generator's by a few per cent.  With FOCAL_LENGTH GlobalReconstructionEstimator.BundleAdjustment() runs
gsfm_ba7_solve, ends below the cost of the NONE run from the same start, writes the focal lengths back where FlattenedTracks() and the
outlier rule read them; with NONE it stores the bytes solver.bundle_adjust returns on the flattened arrays (the behaviour before the option
existed); with a bit the device does not optimise it fails with a message and touches nothing."""
import os
import sys

import numpy as np
import pytest

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd import synth
from globalsfmpy_amd.solver import bundle_adjust, bundle_adjust_focal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))

pytestmark = pytest.mark.gpu
UNESTIMATED_VIEW = 11
FOCAL_ERROR = 0.03   # relative sigma of list.txt's focal lengths about the generator's


@pytest.fixture(scope="module")
def scene():
    return synth.make_tracks(12, 60, 21, lengths=(2, 3, 4, 5, 8, 12), noise_px=0.5, outlier_frac=0.03)


@pytest.fixture(scope="module")
def dataset(scene, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("synthetic_1dsfm_ba7"))
    listed = dict(scene)
    listed["intrinsics"] = scene["intrinsics"].copy()
    listed["intrinsics"][:, 0] *= 1 + FOCAL_ERROR * np.random.default_rng(4).standard_normal(scene["n_cams"])
    ds.write_tracks_dataset(path, listed)
    return path, listed["intrinsics"][:, 0].copy()


def _pipeline_up_to_structure(path, scene, intrinsics):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(path, rec, vg, cov)
    opts = sfm.ReconstructionEstimatorOptions()
    opts.min_num_two_view_inliers = 1
    opts.bundle_adjustment_loss_function_type, opts.bundle_adjustment_robust_loss_width = "HUBER", 10.0
    opts.intrinsics_to_optimize = intrinsics
    est = sfm.GlobalReconstructionEstimator(opts)
    assert est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    rng = np.random.default_rng(9)
    o, p = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    for v in range(scene["n_cams"]):
        if v != UNESTIMATED_VIEW:
            o[v], p[v] = scene["rot_aa"][v], scene["cam_pos"][v] + 0.05 * rng.standard_normal(3)
    sfm.SetReconstructionFromEstimatedPoses(o, p, rec)
    est.EstimateStructure()
    sfm.SetUnderconstrainedAsUnestimated(rec)
    return sfm, est, rec


def _tracks(rec):
    T = rec.NumTracks()
    return np.array([rec.TrackIsEstimated(t) for t in range(T)], np.uint8), np.array([rec.TrackPoint(t) for t in range(T)])


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_none_stores_what_bundle_adjust_returns(dataset, scene):
    path, listed = dataset
    from globalsfmpy_amd import GlobalSfMpy as G
    sfm, est, rec = _pipeline_up_to_structure(path, scene, G.OptimizeIntrinsicsType.NONE)
    flat = rec.FlattenedTracks()
    pt_est, pts0 = _tracks(rec)
    assert np.array_equal(flat["intrinsics"][:, 0], listed)
    w1, c1, p1, s = bundle_adjust(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"], pts0,
                                  flat["cam_estimated"], pt_est, loss=LF.HuberLoss(10.0))
    assert est.BundleAdjustment() is True and est.LastError() == ""
    st = est.LastBundleAdjustmentSummary()
    assert st["ran"] and st["usable"] and st["focal_lengths_free"] is False
    assert (st["termination"], st["num_iterations"], st["num_cg_iterations"], st["final_cost"]) == (s["termination"], s["num_iterations"], s["num_cg_iterations"], s["final_cost"])
    after = rec.FlattenedTracks()
    assert _same_bytes(after["rot_aa"], w1) and _same_bytes(after["cam_pos"], c1) and _same_bytes(_tracks(rec)[1], p1)
    assert _same_bytes(after["intrinsics"], flat["intrinsics"]) and all(rec.ViewFocalLength(int(v)) is None for v in flat["views"])


def test_focal_length_adjusts_writes_back_and_the_outlier_rule_sees_it(dataset, scene):
    path, listed = dataset
    from globalsfmpy_amd import GlobalSfMpy as G
    sfm, est0, rec0 = _pipeline_up_to_structure(path, scene, G.OptimizeIntrinsicsType.NONE)
    sfm, est1, rec1 = _pipeline_up_to_structure(path, scene, G.OptimizeIntrinsicsType.FOCAL_LENGTH)
    flat = rec1.FlattenedTracks()
    pt_est, pts0 = _tracks(rec1)
    for k, v in rec0.FlattenedTracks().items():
        assert np.array_equal(v, flat[k]), k   # the same start
    w1, c1, f1, p1, s = bundle_adjust_focal(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"][:, 0], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"],
                                            flat["obs_xy"], pts0, flat["cam_estimated"], pt_est, loss=LF.HuberLoss(10.0))
    out0 = est0.BundleAdjustmentAndRemoveOutlierPoints()
    out1 = est1.BundleAdjustmentAndRemoveOutlierPoints()
    print("NONE        :", out0)
    print("FOCAL_LENGTH:", out1)
    assert out0["success"] and out1["success"] and out1["usable"] and out1["focal_lengths_free"] is True and out0["focal_lengths_free"] is False
    assert out1["initial_cost"] == out0["initial_cost"] and out1["final_cost"] < out0["final_cost"]
    assert (out1["termination"], out1["num_iterations"], out1["final_cost"]) == (s["termination"], s["num_iterations"], s["final_cost"])
    # written back: ViewFocalLength and FlattenedTracks() show the adjusted focal lengths of the estimated views, the flat call's bytes
    after = rec1.FlattenedTracks()
    est = flat["cam_estimated"].astype(bool)
    assert est.sum() == 11 and _same_bytes(after["intrinsics"][:, 0], f1) and _same_bytes(after["rot_aa"], w1) and _same_bytes(after["cam_pos"], c1)
    for c, v in enumerate(flat["views"]):
        if est[c]:
            assert rec1.ViewFocalLength(int(v)) == f1[c]
        else:
            assert rec1.ViewFocalLength(int(v)) is None and after["intrinsics"][c, 0] == listed[c]
    assert np.all(after["intrinsics"][est, 0] != flat["intrinsics"][est, 0]) and np.array_equal(after["intrinsics"][:, 1:], flat["intrinsics"][:, 1:])
    truth = scene["intrinsics"][:, 0]
    err0, err1 = np.abs(listed / truth - 1)[est], np.abs(f1 / truth - 1)[est]
    print("relative focal error: listed median %.4f max %.4f, adjusted median %.4f max %.4f" % (np.median(err0), err0.max(), np.median(err1), err1.max()))
    assert np.median(err1) < np.median(err0)
    # the outlier rule that follows read them: it removes no more tracks than with the listed focal lengths held
    assert out1["num_points_removed"] <= out0["num_points_removed"]
    assert est1.LastOutlierSummary()["num_examined"] == est0.LastOutlierSummary()["num_examined"]
    # and so does the next structure call: the flattened arrays it runs on carry them
    est1.EstimateStructure(only_unestimated=True)
    assert _same_bytes(rec1.FlattenedTracks()["intrinsics"][:, 0], f1)
    # BundleAdjustCameraPositionsAndPoints holds the intrinsics whatever the option says
    assert est1.BundleAdjustCameraPositionsAndPoints() is True and est1.LastBundleAdjustmentSummary()["focal_lengths_free"] is False
    assert _same_bytes(rec1.FlattenedTracks()["intrinsics"][:, 0], f1)


def test_an_unsupported_bit_fails_with_a_message_and_touches_nothing(dataset, scene):
    path, _ = dataset
    from globalsfmpy_amd import GlobalSfMpy as G
    T = G.OptimizeIntrinsicsType
    sfm, est, rec = _pipeline_up_to_structure(path, scene, T.FOCAL_LENGTH | T.RADIAL_DISTORTION)
    flat0, (pt0, pts0) = rec.FlattenedTracks(), _tracks(rec)
    assert est.BundleAdjustment() is False
    assert "RADIAL_DISTORTION" in est.LastError() and est.LastBundleAdjustmentSummary()["ran"] is False
    flat1, (pt1, pts1) = rec.FlattenedTracks(), _tracks(rec)
    for k in flat0:
        assert _same_bytes(flat0[k], flat1[k]), k
    assert _same_bytes(pt0, pt1) and _same_bytes(pts0, pts1)
    est.options.intrinsics_to_optimize = T.FOCAL_LENGTH   # the same estimator goes on once the option is one it runs
    assert est.BundleAdjustment() is True and est.LastError() == "" and est.LastBundleAdjustmentSummary()["focal_lengths_free"] is True
