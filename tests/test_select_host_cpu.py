"""The track selection's options and bindings in the module (no device): the four defaults are Theia's header defaults, load_1DSFM_config
reads the four YAML keys, and the new names exist."""
import os
import sys

from globalsfmpy_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))

KEYS = ("subsample_tracks_for_bundle_adjustment", "track_subset_selection_long_track_length_threshold", "track_selection_image_grid_cell_size_pixels",
        "min_num_optimized_tracks_per_view")


def test_option_defaults_are_theia_s_header_defaults():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    o = sfm.ReconstructionEstimatorOptions()
    assert [getattr(o, k) for k in KEYS] == [False, 10, 100, 200]
    assert [getattr(sfm.ReconstructionBuilderOptions().reconstruction_estimator_options, k) for k in KEYS] == [False, 10, 100, 200]
    for k, v in zip(KEYS, (True, 3, 25, 7)):
        setattr(o, k, v)
    assert [getattr(o, k) for k in KEYS] == [True, 3, 25, 7]


def test_the_four_yaml_keys_are_read(tmp_path):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    flags = tmp_path / "flags.yaml"
    # the values of the reference's flag files, but for the switch
    flags.write_text("subsample_tracks_for_bundle_adjustment: true\ntrack_subset_selection_long_track_length_threshold: 10\n"
                     "track_selection_image_grid_cell_size_pixels: 100\nmin_num_optimized_tracks_per_view: 100\n")
    b = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), b)
    assert [getattr(b.reconstruction_estimator_options, k) for k in KEYS] == [True, 10, 100, 100]
    flags.write_text("track_subset_selection_long_track_length_threshold: 4\ntrack_selection_image_grid_cell_size_pixels: 64\n")
    b = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), b)
    assert [getattr(b.reconstruction_estimator_options, k) for k in KEYS] == [False, 4, 64, 200]     # an absent key keeps its default


def test_the_new_names_exist():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    assert callable(sfm.SelectGoodTracksForBundleAdjustment) and hasattr(sfm.GlobalReconstructionEstimator, "LastTrackSelection")
    assert callable(solver.select_good_tracks) and callable(solver.select_good_tracks_from_statistics)
    assert solver.TRACK_SELECT_COUNTS == ("tracks_with_items", "cells", "selected_by_cell", "cameras_topped_up", "selected_by_top_up", "selected")
    d = sfm.GlobalReconstructionEstimator(sfm.ReconstructionEstimatorOptions()).LastTrackSelection()
    assert d["ran"] is False and all(d[k] == 0 for k in solver.TRACK_SELECT_COUNTS) and d["kernel_ms"] == 0.0
    assert {"long_track_length_threshold", "image_grid_cell_size_pixels", "min_num_optimized_tracks_per_view"} <= set(d)


def test_a_reconstruction_without_tracks_selects_nothing():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    assert sfm.SelectGoodTracksForBundleAdjustment(sfm.Reconstruction(), 10, 100, 200) == []
