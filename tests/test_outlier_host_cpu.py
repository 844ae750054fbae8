"""The host side of the structure loop without a device: the three options that drive it (defaults and YAML keys), the new bindings' names,
and the sub-CSR of the unestimated tracks that EstimateStructure(only_unestimated=True) runs, on a hand-made reconstruction."""
import os
import sys

import numpy as np

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))

TRACKS = [[0, 1, 2], [3, 4], [0, 5, 1, 2], [4, 0], [2, 3, 5, 1, 0]]


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


def _reconstruction(tmp_path):
    sfm = _sfm()
    base = synth.make_tracks(6, 1, 3, lengths=(2,), noise_px=0.0)
    g = {k: base[k] for k in ("n_cams", "rot_aa", "cam_pos", "intrinsics")}
    g["obs_cam"] = np.concatenate(TRACKS).astype(np.uint32)
    g["track_ptr"] = np.concatenate([[0], np.cumsum([len(t) for t in TRACKS])]).astype(np.uint64)
    g["obs_xy"] = np.arange(2 * len(g["obs_cam"]), dtype=float).reshape(-1, 2) + 0.25
    ds.write_tracks_dataset(str(tmp_path), g)
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(str(tmp_path), rec, vg, cov)
    o, p = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    for v in range(6):
        o[v], p[v] = g["rot_aa"][v], g["cam_pos"][v]
    sfm.SetReconstructionFromEstimatedPoses(o, p, rec)
    return sfm, rec, g


def test_option_defaults_are_theias():
    o = _sfm().ReconstructionEstimatorOptions()
    assert o.max_reprojection_error_in_pixels == 5.0 and o.num_retriangulation_iterations == 1
    assert o.refine_camera_positions_and_points_after_position_estimation is True
    assert o.triangulation_max_reprojection_error_in_pixels == 15.0          # the triangulation's own bound is another option


def test_yaml_keys_are_read(tmp_path):
    sfm = _sfm()
    flags = tmp_path / "flags.yaml"
    flags.write_text("max_reprojection_error_pixels: 3.5\nnum_retriangulation_iterations: 0\n"
                     "refine_camera_positions_and_points_after_position_estimation: false\n")
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts)
    o = opts.reconstruction_estimator_options
    assert o.max_reprojection_error_in_pixels == 3.5 and o.num_retriangulation_iterations == 0
    assert o.refine_camera_positions_and_points_after_position_estimation is False
    assert o.triangulation_max_reprojection_error_in_pixels == 15.0
    # a file without the keys leaves the defaults
    flags.write_text("num_threads: 2\n")
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts)
    o = opts.reconstruction_estimator_options
    assert (o.max_reprojection_error_in_pixels, o.num_retriangulation_iterations) == (5.0, 1)
    assert o.refine_camera_positions_and_points_after_position_estimation is True


def test_new_names_exist():
    sfm = _sfm()
    e = sfm.GlobalReconstructionEstimator(sfm.ReconstructionEstimatorOptions())
    assert hasattr(e, "BundleAdjustmentAndRemoveOutlierPoints") and hasattr(e, "LastOutlierSummary")
    assert hasattr(sfm, "SetOutlierTracksToUnestimated")
    assert e.LastOutlierSummary() == {"num_examined": 0, "num_removed": 0, "kernel_ms": 0.0, "counts": [0, 0, 0, 0, 0],
                                      "num_bad_reprojections": 0, "num_insufficient_viewing_angles": 0}
    assert "only_unestimated" in e.EstimateStructure.__doc__
    # a reconstruction without tracks is left alone, with or without a device
    rec = sfm.Reconstruction()
    rec.SetOrientation(0, np.zeros(3))
    assert sfm.SetOutlierTracksToUnestimated(5.0, 4.0, rec) == 0


def test_sub_csr_of_the_unestimated_tracks(tmp_path):
    sfm, rec, g = _reconstruction(tmp_path)
    full = rec.FlattenedTracks()
    assert "track_index" not in full and np.array_equal(full["track_ptr"], g["track_ptr"])
    # nothing estimated yet: every track, in order
    sub = rec.FlattenedTracks(only_unestimated=True)
    assert list(sub["track_index"]) == [0, 1, 2, 3, 4]
    for k in ("track_ptr", "obs_cam", "obs_xy"):
        assert np.array_equal(sub[k], full[k]), k
    # tracks 1 and 3 estimated: the sub-batch is 0, 2, 4 with their own slices
    rec.SetTrack(1, np.array([1.0, 2.0, 3.0]), True)
    rec.SetTrack(3, np.array([4.0, 5.0, 6.0]), True)
    rec.SetTrack(4, np.array([7.0, 8.0, 9.0]), False)
    sub = rec.FlattenedTracks(only_unestimated=True)
    assert list(sub["track_index"]) == [0, 2, 4] and sub["track_index"].dtype == np.uint64
    assert list(sub["track_ptr"]) == [0, 3, 7, 12] and sub["track_ptr"].dtype == np.uint64
    assert list(sub["obs_cam"]) == TRACKS[0] + TRACKS[2] + TRACKS[4]
    ptr = g["track_ptr"].astype(np.int64)
    want_xy = np.vstack([full["obs_xy"][ptr[t]:ptr[t + 1]] for t in (0, 2, 4)])
    assert sub["obs_xy"].shape == (12, 2) and np.array_equal(sub["obs_xy"], want_xy)
    for k in ("views", "rot_aa", "cam_pos", "intrinsics", "cam_estimated"):          # the cameras stay
        assert np.array_equal(sub[k], full[k]), k
    assert np.array_equal(rec.FlattenedTracks()["track_ptr"], g["track_ptr"])         # the default is unchanged
    # every track estimated: an empty sub-batch
    for t in (0, 2, 4):
        rec.SetTrack(t, np.zeros(3), True)
    sub = rec.FlattenedTracks(only_unestimated=True)
    assert len(sub["track_index"]) == 0 and list(sub["track_ptr"]) == [0] and len(sub["obs_cam"]) == 0 and sub["obs_xy"].size == 0
