"""The host layer of the per-track refinement on a synthetic 1DSfM dataset: GlobalReconstructionEstimator.EstimateStructure(refine=True)
honours bundle_adjust_tracks and stores for every track exactly what the flat-array call with refine=True returns on the arrays
Reconstruction.FlattenedTracks() shows; with the option off it stores the unrefined result; the default call is what it was."""
import os
import sys

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd.solver import triangulate_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives, as the reference's scripts append ../build

pytestmark = pytest.mark.gpu

UNESTIMATED_VIEW = 11


@pytest.fixture(scope="module")
def scene():
    return synth.make_tracks(12, 60, 21, lengths=(2, 3, 4, 5, 8, 12), noise_px=0.5, outlier_frac=0.03)


@pytest.fixture(scope="module")
def dataset(scene, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("synthetic_1dsfm_refined_tracks"))
    ds.write_tracks_dataset(path, scene)
    return path


def estimator_with_ground_truth_poses(sfm, path, scene):
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(path, rec, vg, cov)
    opts = sfm.ReconstructionEstimatorOptions()
    opts.min_num_two_view_inliers = 1
    est = sfm.GlobalReconstructionEstimator(opts)
    assert est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    o, p = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    for v in range(scene["n_cams"]):
        if v != UNESTIMATED_VIEW:
            o[v], p[v] = scene["rot_aa"][v], scene["cam_pos"][v]
    sfm.SetReconstructionFromEstimatedPoses(o, p, rec)
    return est, rec


def flat_call(flat, **kw):
    return triangulate_tracks(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"],
                              cam_estimated=flat["cam_estimated"], min_triangulation_angle_degrees=4.0, max_reprojection_error_pixels=15.0, **kw)


def stored_equals(rec, ref):
    T = len(ref["status"])
    return all(rec.TrackIsEstimated(t) == (ref["status"][t] == 0) and
               np.array_equal(np.array(rec.TrackPoint(t)).view(np.uint64), ref["points"][t].view(np.uint64)) for t in range(T))


def test_refined_structure_is_the_flat_call_and_the_default_call_is_unchanged(dataset, scene):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    est, rec = estimator_with_ground_truth_poses(sfm, dataset, scene)
    T = len(scene["track_ptr"]) - 1
    flat = rec.FlattenedTracks()
    assert est.options.bundle_adjust_tracks is True and est.options.bundle_adjustment_loss_function_type == "TRIVIAL"
    assert est.options.bundle_adjustment_robust_loss_width == 10.0
    plain = flat_call(flat)
    # the default call: today's dict, today's points
    stats0 = est.EstimateStructure()
    assert sorted(stats0) == ["bundle_adjust_tracks_requested", "counts", "kernel_ms", "note", "num_bad_angles", "num_bad_reprojections", "num_estimated",
                              "num_failed_triangulations", "num_tracks", "tracks_refined"]
    assert stats0["tracks_refined"] is False and stats0["note"] == "tracks triangulated without per-track refinement (bundle_adjust_tracks is not honoured)"
    assert list(stats0["counts"]) == [int(c) for c in plain["counts"]] and stored_equals(rec, plain)
    # refine=True, once per loss the YAML can name
    for name, loss in (("TRIVIAL", [(_abi.LOSS_TRIVIAL,)]), ("HUBER", [(_abi.LOSS_HUBER, 10.0)])):
        est.options.bundle_adjustment_loss_function_type = name
        ref = flat_call(flat, refine=True, loss=loss)
        stats = est.EstimateStructure(refine=True)
        print("EstimateStructure(refine=True), %s: %s" % (name, stats))
        assert stats["tracks_refined"] is True and stats["bundle_adjust_tracks_requested"] is True and "refined per track" in stats["note"]
        assert stats["num_tracks"] == T and stats["num_estimated"] == int(np.sum(ref["status"] == 0)) == rec.NumEstimatedTracks()
        assert list(stats["counts"]) == [int(c) for c in ref["counts"][:6]] and stats["num_refinement_failed"] == int(ref["counts"][6])
        done = ref["termination"] >= 0
        assert stats["max_iterations"] == int(ref["iterations"].max()) and abs(stats["mean_iterations"] - ref["iterations"][done].mean()) < 1e-12
        assert stored_equals(rec, ref) and est.LastStructureSummary() == stats
        good = np.flatnonzero(ref["status"] == 0)
        assert not stored_equals(rec, plain) and np.max(np.linalg.norm(ref["points"][good] - scene["gt_points"][good], axis=1)) < 0.2
    # the option off: the unrefined result, and the dict says so
    est.options.bundle_adjust_tracks = False
    off = est.EstimateStructure(refine=True)
    assert off["tracks_refined"] is False and off["bundle_adjust_tracks_requested"] is False and off["num_refinement_failed"] == 0
    assert list(off["counts"]) == [int(c) for c in plain["counts"]] and stored_equals(rec, plain)
    est.options.bundle_adjust_tracks = True
    est.options.bundle_adjustment_loss_function_type = "CAUCHY"
    with pytest.raises(RuntimeError, match="no loss CAUCHY"):
        est.EstimateStructure(refine=True)


def test_yaml_names_the_loss(tmp_path):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    flags = tmp_path / "flags.yaml"
    flags.write_text("bundle_adjust_tracks: true\nbundle_adjustment_robust_loss_function: HUBER\nbundle_adjustment_robust_loss_width: 7.5\n")
    options = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), options)
    o = options.reconstruction_estimator_options
    assert o.bundle_adjust_tracks is True and o.bundle_adjustment_loss_function_type == "HUBER" and o.bundle_adjustment_robust_loss_width == 7.5
