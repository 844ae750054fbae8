"""-m gpu: the track selection in the host layer, on the synthetic 1DSfM dataset of test_gpu_ba_host.py (12 cameras, 60 tracks) and on that of
the position pipeline's test (12 cameras, 600 points).  With subsample_tracks_for_bundle_adjustment unset both bundle adjustments leave the
reconstruction in the bytes of an estimator that never heard of the options; with it set sfm.SelectGoodTracksForBundleAdjustment returns what
solver.select_good_tracks marks, BundleAdjustment() drops every estimated track that was not chosen and adjusts the rest, and
BundleAdjustCameraPositionsAndPoints() moves the chosen points alone and touches no flag."""
import importlib.util
import os

import numpy as np
import pytest

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import bundle_adjust_positions_and_points, select_good_tracks

from test_gpu_ba_host import _pipeline_up_to_structure, dataset, scene  # noqa: F401  (the fixtures and the pipeline of the bundle-adjustment tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S, K = 10, 500, 3   # cells of 500 pixels: a few per camera, so that the subset is proper on 60 tracks

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float64)).view(np.uint64)


def _state(rec):
    """every pose, point and flag of a reconstruction, as bytes"""
    T = rec.NumTracks()
    rot, pos = rec.EstimatedOrientations(), rec.EstimatedPositions()
    return {"rot": {int(v): _bits(w).tobytes() for v, w in rot.items()}, "pos": {int(v): _bits(p).tobytes() for v, p in pos.items()},
            "points": [_bits(rec.TrackPoint(t)).tobytes() for t in range(T)], "flags": [rec.TrackIsEstimated(t) for t in range(T)]}


def _ready(dataset, scene, subsample):  # noqa: F811
    sfm, est, rec = _pipeline_up_to_structure(dataset, scene)
    sfm.SetUnderconstrainedAsUnestimated(rec)
    o = est.options
    o.track_subset_selection_long_track_length_threshold, o.track_selection_image_grid_cell_size_pixels, o.min_num_optimized_tracks_per_view = L, S, K
    o.subsample_tracks_for_bundle_adjustment = subsample
    return sfm, est, rec


def _flat_selection(rec):
    T = rec.NumTracks()
    flat = rec.FlattenedTracks()
    flags = np.array([rec.TrackIsEstimated(t) for t in range(T)], np.uint8)
    pts = np.array([rec.TrackPoint(t) for t in range(T)])
    sel = select_good_tracks(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"], pts,
                             cam_estimated=flat["cam_estimated"], point_estimated=flags, long_track_length_threshold=L, image_grid_cell_size_pixels=S,
                             min_num_optimized_tracks_per_view=K)
    return flat, flags, pts, sel


@pytest.mark.parametrize("method", ["BundleAdjustment", "BundleAdjustCameraPositionsAndPoints"])
def test_with_the_flag_unset_nothing_changes(dataset, scene, method):  # noqa: F811
    sfm, est_a, rec_a = _ready(dataset, scene, False)
    _, est_b, rec_b = _pipeline_up_to_structure(dataset, scene)      # an estimator that never heard of the options
    sfm.SetUnderconstrainedAsUnestimated(rec_b)
    assert _state(rec_a) == _state(rec_b)
    assert getattr(est_a, method)() is True and getattr(est_b, method)() is True
    assert _state(rec_a) == _state(rec_b)
    a, b = est_a.LastBundleAdjustmentSummary(), est_b.LastBundleAdjustmentSummary()
    assert all(a[k] == b[k] for k in a if k != "t_total_ms")
    d = est_a.LastTrackSelection()
    assert d["ran"] is False and d["selected"] == 0 and d["kernel_ms"] == 0.0


def test_module_function_returns_what_the_flat_call_marks(dataset, scene):  # noqa: F811
    sfm, est, rec = _ready(dataset, scene, True)
    before = _state(rec)
    flat, flags, pts, sel = _flat_selection(rec)
    chosen = sfm.SelectGoodTracksForBundleAdjustment(rec, L, S, K)
    print("selection on the 60-track dataset (L, S, K = %d, %d, %d): %s" % (L, S, K, sel["counts"]))
    assert chosen == sorted(chosen) and chosen == [int(t) for t in np.flatnonzero(sel["selected"])]
    assert 0 < len(chosen) < int(flags.sum())                          # a proper subset of the estimated tracks
    assert all(flags[t] for t in chosen)
    assert _state(rec) == before                                       # the selection changes nothing


def test_bundle_adjustment_keeps_exactly_the_chosen_tracks(dataset, scene):  # noqa: F811
    sfm, est, rec = _ready(dataset, scene, True)
    T = rec.NumTracks()
    before = _state(rec)
    _, flags, _, sel = _flat_selection(rec)
    chosen = sel["selected"] != 0
    assert est.BundleAdjustment() is True
    after = _state(rec)
    assert after["flags"] == [bool(c) for c in chosen] and 0 < chosen.sum() < flags.sum()
    st, d = est.LastBundleAdjustmentSummary(), est.LastTrackSelection()
    print("BundleAdjustment on the subset: %s; selection %s" % (st, d))
    assert st["ran"] and st["usable"] and st["num_points"] == int(chosen.sum()) and st["final_cost"] <= st["initial_cost"]
    assert d["ran"] is True and d["selected"] == int(chosen.sum()) and {k: d[k] for k in sel["counts"]} == sel["counts"] and d["kernel_ms"] > 0
    assert (d["long_track_length_threshold"], d["image_grid_cell_size_pixels"], d["min_num_optimized_tracks_per_view"]) == (L, S, K)
    for t in range(T):                                                 # the tracks that were dropped keep their points
        if not chosen[t]:
            assert after["points"][t] == before["points"][t], t
    assert any(after["points"][t] != before["points"][t] for t in np.flatnonzero(chosen))
    # the flags stay cleared: the outlier rule examines the chosen tracks alone
    sfm.SetOutlierTracksToUnestimated(5.0, 4.0, rec)
    assert all(not f for f, c in zip(_state(rec)["flags"], chosen) if not c)


def test_positions_and_points_moves_the_chosen_points_alone(dataset, scene):  # noqa: F811
    sfm, est, rec = _ready(dataset, scene, True)
    T = rec.NumTracks()
    before = _state(rec)
    flat, flags, pts, sel = _flat_selection(rec)
    chosen = sel["selected"] != 0
    c1, p1, s = bundle_adjust_positions_and_points(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"],
                                                   pts, flat["cam_estimated"], (flags != 0) & chosen, loss=LF.HuberLoss(10.0))
    assert est.BundleAdjustCameraPositionsAndPoints() is True
    after = _state(rec)
    st = est.LastBundleAdjustmentSummary()
    assert after["flags"] == before["flags"] and after["rot"] == before["rot"]                 # every flag is as before
    assert st["num_points"] == int(chosen.sum()) and (st["termination"], st["num_iterations"]) == (s["termination"], s["num_iterations"])
    assert st["initial_cost"] == s["initial_cost"] and st["final_cost"] == s["final_cost"]
    for t in range(T):
        if chosen[t]:
            assert after["points"][t] == _bits(p1[t]).tobytes(), t
        else:
            assert after["points"][t] == before["points"][t], t
    for c, v in enumerate(flat["views"]):
        if flat["cam_estimated"][c]:
            assert after["pos"][int(v)] == _bits(c1[c]).tobytes(), v
    assert est.LastTrackSelection()["ran"] is True and est.LastTrackSelection()["selected"] == int(chosen.sum())


@pytest.fixture(scope="module")
def pipeline_dataset(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("synthetic_1dsfm_selection"))
    ds.write_synthetic_dataset(path, n_cams=12, n_points=600, seed=3)
    return path


def _example():
    spec = importlib.util.spec_from_file_location("reconstruction_pipeline_example", os.path.join(ROOT, "examples", "reconstruction_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_options_flow_through_the_example_pipeline(pipeline_dataset, tmp_path):
    flags = tmp_path / "flags.yaml"
    flags.write_text("num_retriangulation_iterations: 0\nsubsample_tracks_for_bundle_adjustment: true\ntrack_subset_selection_long_track_length_threshold: 10\n"
                     "track_selection_image_grid_cell_size_pixels: 200\nmin_num_optimized_tracks_per_view: 20\n")
    rec, est, passes = _example().run_pipeline(pipeline_dataset, str(flags))
    d = est.LastTrackSelection()
    print("selection in the example pipeline (600 points): %s" % d)
    assert d["ran"] is True and (d["image_grid_cell_size_pixels"], d["min_num_optimized_tracks_per_view"]) == (200, 20)
    assert 0 < d["selected"] < d["tracks_with_items"]                  # a proper subset went to the last adjustment
    assert passes[0]["bundle_adjustment"]["success"] is True and passes[0]["bundle_adjustment"]["num_points"] == d["selected"]
    # the tracks that were not chosen are unestimated for good: what is left after the outlier step comes out of the chosen ones
    assert passes[0]["estimated_after_outlier_step"] == d["selected"] - passes[0]["bundle_adjustment"]["num_points_removed"]
    assert passes[0]["estimated_before_outlier_step"] > d["selected"]
    plain = tmp_path / "plain.yaml"
    plain.write_text("num_retriangulation_iterations: 0\n")
    rec0, est0, passes0 = _example().run_pipeline(pipeline_dataset, str(plain))
    assert est0.LastTrackSelection()["ran"] is False
    assert passes0[0]["bundle_adjustment"]["num_points"] > d["selected"]
