"""-m gpu: the host layer of the structure loop on the synthetic 1DSfM dataset of test_gpu_triangulation_host.py / test_gpu_ba_host.py (12
cameras, 60 tracks): sfm.SetOutlierTracksToUnestimated clears exactly the flags solver.outlier_tracks marks; BundleAdjustmentAndRemoveOutlierPoints()
is BundleAdjustment() followed by it, and removes nothing after an unusable adjustment; EstimateStructure(only_unestimated=True) leaves the
estimated tracks alone and gives every other track what a call over all tracks gives it.  examples/reconstruction_pipeline.py runs on the
dataset of the position pipeline's test (12 cameras, 600 points): the 60-track one has no view pair with the default 30 verified matches."""
import importlib.util
import os

import numpy as np
import pytest

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd.solver import outlier_tracks

from test_gpu_ba_host import UNESTIMATED_VIEW, _pipeline_up_to_structure, dataset, scene  # noqa: F401  (the fixtures and the pipeline of the bundle-adjustment tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float64)).view(np.uint64)


def _state(rec):
    """every pose, point and flag of a reconstruction, as bytes"""
    T = rec.NumTracks()
    rot, pos = rec.EstimatedOrientations(), rec.EstimatedPositions()
    return {"rot": {int(v): _bits(w).tobytes() for v, w in rot.items()}, "pos": {int(v): _bits(p).tobytes() for v, p in pos.items()},
            "points": [_bits(rec.TrackPoint(t)).tobytes() for t in range(T)], "flags": [rec.TrackIsEstimated(t) for t in range(T)]}


@pytest.mark.parametrize("max_err", [5.0, 1.0])
def test_module_function_clears_what_the_flat_call_marks(dataset, scene, max_err):  # noqa: F811
    sfm, est, rec = _pipeline_up_to_structure(dataset, scene)
    T = rec.NumTracks()
    flat = rec.FlattenedTracks()
    before = _state(rec)
    pts = np.array([rec.TrackPoint(t) for t in range(T)])
    flags = np.array(before["flags"], np.uint8)
    ref = outlier_tracks(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"], pts,
                         cam_estimated=flat["cam_estimated"], point_estimated=flags, max_reprojection_error_pixels=max_err,
                         min_triangulation_angle_degrees=4.0)
    marked = ref["status"] >= 2
    assert (ref["status"][flags == 0] == 1).all() and not marked[flags == 0].any()
    removed = sfm.SetOutlierTracksToUnestimated(max_err, 4.0, rec)
    after = _state(rec)
    print("max_err %.1f: %d of %d estimated tracks removed, statuses %s" % (max_err, removed, int(flags.sum()), ref["counts"]))
    assert isinstance(removed, int) and removed == int(marked.sum()) == sum(b and not a for a, b in zip(after["flags"], before["flags"]))
    assert after["flags"] == [bool(f) and not m for f, m in zip(flags, marked)]
    assert after["points"] == before["points"] and after["rot"] == before["rot"] and after["pos"] == before["pos"]     # nothing moves
    if max_err == 1.0:      # the cameras stand 0.05 off and the pixels carry 0.5 px of noise: a 1 px bound removes tracks, and keeps some
        assert 1 <= removed < int(flags.sum())
    assert sfm.SetOutlierTracksToUnestimated(max_err, 4.0, rec) == 0                                                  # nothing left to remove


def test_estimator_method_is_the_adjustment_followed_by_the_module_function(dataset, scene):  # noqa: F811
    sfm, est_a, rec_a = _pipeline_up_to_structure(dataset, scene)
    _, est_b, rec_b = _pipeline_up_to_structure(dataset, scene)
    for est, rec in ((est_a, rec_a), (est_b, rec_b)):
        sfm.SetUnderconstrainedAsUnestimated(rec)
        est.options.max_reprojection_error_in_pixels = 0.7           # the pixels carry 0.5 px of noise per coordinate: some tracks go, some stay
    assert _state(rec_a) == _state(rec_b)
    d = est_a.BundleAdjustmentAndRemoveOutlierPoints()
    assert est_b.BundleAdjustment() is True
    n = sfm.SetOutlierTracksToUnestimated(est_b.options.max_reprojection_error_in_pixels, est_b.options.min_triangulation_angle_degrees, rec_b)
    print("BundleAdjustmentAndRemoveOutlierPoints: %s; outliers %s" % (d, est_a.LastOutlierSummary()))
    assert _state(rec_a) == _state(rec_b)
    assert d["success"] is True and d["num_points_removed"] == n and 1 <= n < est_a.LastOutlierSummary()["num_examined"]
    summary = est_a.LastBundleAdjustmentSummary()
    assert {k: v for k, v in d.items() if k not in ("success", "num_points_removed")} == summary and summary["ran"] and summary["usable"]
    other = est_b.LastBundleAdjustmentSummary()
    assert all(summary[k] == other[k] for k in summary if k != "t_total_ms")
    o = est_a.LastOutlierSummary()
    assert o["num_removed"] == n == o["counts"][2] + o["counts"][3] + o["counts"][4] == o["num_bad_reprojections"] + o["num_insufficient_viewing_angles"]
    assert o["num_examined"] == sum(o["counts"]) - o["counts"][1] and o["num_examined"] - n == rec_a.NumEstimatedTracks() and o["kernel_ms"] > 0
    assert est_b.LastOutlierSummary()["num_examined"] == 0          # the module function is not the estimator's


def test_an_unusable_adjustment_removes_nothing(dataset, scene):  # noqa: F811
    """FAILURE is the one unusable termination (an adjustment stopped at its iteration limit is NO_CONVERGENCE, which is usable), so a
    non-finite point is planted: the initial cost is not finite"""
    sfm, est, rec = _pipeline_up_to_structure(dataset, scene)
    _, twin_est, twin = _pipeline_up_to_structure(dataset, scene)
    for e, r in ((est, rec), (twin_est, twin)):
        sfm.SetUnderconstrainedAsUnestimated(r)
        e.options.max_reprojection_error_in_pixels = 0.0             # a bound every noisy track misses: after a usable adjustment all of them go
    flags = _state(rec)["flags"]
    assert sum(flags) >= 30
    d = twin_est.BundleAdjustmentAndRemoveOutlierPoints()
    assert d["success"] is True and d["usable"] is True and d["num_points_removed"] == sum(flags) and twin.NumEstimatedTracks() == 0
    t = flags.index(True)
    rec.SetTrack(t, np.array([np.nan, 0.0, 1.0]), True)              # a non-finite point: the initial cost is not finite, FAILURE
    d = est.BundleAdjustmentAndRemoveOutlierPoints()
    print("after a planted non-finite point: %s" % d)
    assert d["success"] is False and d["usable"] is False and d["ran"] is True and d["num_points_removed"] == 0
    assert _state(rec)["flags"] == flags
    assert est.LastOutlierSummary()["num_examined"] == 0 and est.LastOutlierSummary()["kernel_ms"] == 0.0


@pytest.mark.parametrize("refine", [False, True])
def test_only_unestimated_leaves_estimated_tracks_and_matches_a_full_call_elsewhere(dataset, scene, refine):  # noqa: F811
    sfm, est_a, rec_a = _pipeline_up_to_structure(dataset, scene)
    _, est_b, rec_b = _pipeline_up_to_structure(dataset, scene)
    T = rec_a.NumTracks()
    flags = _state(rec_a)["flags"]
    estimated = [t for t in range(T) if flags[t]]
    assert len(estimated) >= 30 and len(estimated) < T
    dropped = estimated[::5]                                          # estimated tracks that lose their flag and get a junk point: retriangulated
    kept = [t for t in estimated if t not in dropped]
    for t in kept:
        rec_a.SetTrack(t, np.array([1000.0 + t, -float(t), 0.5]), True)      # sentinels
    for t in dropped:
        rec_a.SetTrack(t, np.array([-7.0, -7.0, -7.0]), False)
    sub = rec_a.FlattenedTracks(only_unestimated=True)
    others = [t for t in range(T) if t not in kept]
    assert list(sub["track_index"]) == others
    stats = est_a.EstimateStructure(refine=refine, only_unestimated=True)
    full = est_b.EstimateStructure(refine=refine)
    print("only_unestimated (refine=%s): %s" % (refine, stats))
    for t in kept:
        assert rec_a.TrackIsEstimated(t) and np.array_equal(_bits(rec_a.TrackPoint(t)), _bits([1000.0 + t, -float(t), 0.5])), t
    for t in others:
        assert rec_a.TrackIsEstimated(t) == rec_b.TrackIsEstimated(t), t
        assert np.array_equal(_bits(rec_a.TrackPoint(t)), _bits(rec_b.TrackPoint(t))), t
    assert all(rec_a.TrackIsEstimated(t) for t in dropped) or refine          # the midpoint call accepted them before
    assert stats["num_tracks"] == len(others) and stats["num_estimated"] == sum(rec_a.TrackIsEstimated(t) for t in others)
    assert sum(stats["counts"]) + (stats["num_refinement_failed"] if refine else 0) == len(others) and stats["kernel_ms"] > 0
    assert full["num_tracks"] == T and stats["tracks_refined"] is refine
    # nothing left to triangulate: no device work, nothing changes
    for t in range(T):
        rec_a.SetTrack(t, np.array(rec_a.TrackPoint(t)), True)
    before = _state(rec_a)
    stats = est_a.EstimateStructure(refine=refine, only_unestimated=True)
    assert stats["num_tracks"] == 0 and stats["kernel_ms"] == 0.0 and _state(rec_a) == before


@pytest.fixture(scope="module")
def pipeline_dataset(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("synthetic_1dsfm_reconstruction"))
    ds.write_synthetic_dataset(path, n_cams=12, n_points=600, seed=3)
    return path


def _example():
    spec = importlib.util.spec_from_file_location("reconstruction_pipeline_example", os.path.join(ROOT, "examples", "reconstruction_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_pipeline_runs_through_with_the_default_options(pipeline_dataset):
    rec, est, passes = _example().run_pipeline(pipeline_dataset)
    assert est.options.num_retriangulation_iterations == 1 and len(passes) == 2
    assert "positions_and_points" in passes[0] and "positions_and_points" not in passes[1]       # the partial adjustment on pass 0 only
    for i, p in enumerate(passes):
        print("pass %d: structure %s; outliers %s; %d -> %d estimated tracks"
              % (i, p["structure"], p["outliers"], p["estimated_before_outlier_step"], p["estimated_after_outlier_step"]))
        assert p["bundle_adjustment"]["success"] is True
        assert p["estimated_after_outlier_step"] == p["estimated_before_outlier_step"] - p["bundle_adjustment"]["num_points_removed"]
        assert p["estimated_after_outlier_step"] <= p["estimated_before_outlier_step"]           # an outlier step never adds a track
    # the second pass triangulates only what the first left unestimated
    assert passes[1]["structure"]["num_tracks"] == rec.NumTracks() - passes[0]["estimated_after_outlier_step"]
    assert rec.NumEstimatedTracks() >= 10
    assert all(np.all(np.isfinite(np.array(rec.TrackPoint(t)))) for t in rec.EstimatedTrackIds())
    poses = list(rec.EstimatedOrientations().values()) + list(rec.EstimatedPositions().values())
    assert len(poses) >= 12 and all(np.all(np.isfinite(np.array(p))) for p in poses)


def test_example_pipeline_without_retriangulation_runs_the_loop_once(pipeline_dataset, tmp_path):
    flags = tmp_path / "flags.yaml"
    flags.write_text("num_retriangulation_iterations: 0\nrefine_camera_positions_and_points_after_position_estimation: false\n")
    rec, est, passes = _example().run_pipeline(pipeline_dataset, str(flags))
    assert len(passes) == 1 and "positions_and_points" not in passes[0]
    assert passes[0]["structure"]["num_tracks"] == rec.NumTracks()                               # nothing was estimated before the first pass
    assert rec.NumEstimatedTracks() == passes[0]["estimated_after_outlier_step"] >= 10
