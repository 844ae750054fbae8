"""SetUnderconstrainedAsUnestimated (host code, Theia's rule) on a hand-made reconstruction that needs more than one round: views with
fewer than 3 estimated tracks, then tracks with fewer than 2 estimated views, alternating until either pass changes nothing."""
import os
import sys

import numpy as np

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))

# views 0 .. 3 share four tracks.  View 5 sees two tracks only: round 1 drops it, and with it tracks 6 and 7 (one view left each).  View 4
# then sees two estimated tracks (4, 5): round 2 drops it and tracks 4 and 5.  Round 3 finds no view to drop and stops.  Track 8 was never estimated.
TRACKS = [[0, 1, 2, 3]] * 4 + [[4, 0], [4, 1], [4, 5], [5, 0], [2, 3]]


def _reconstruction(tmp_path):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    base = synth.make_tracks(6, 1, 3, lengths=(2,), noise_px=0.0)
    g = {k: base[k] for k in ("n_cams", "rot_aa", "cam_pos", "intrinsics")}
    g["obs_cam"] = np.concatenate(TRACKS).astype(np.uint32)
    g["track_ptr"] = np.concatenate([[0], np.cumsum([len(t) for t in TRACKS])]).astype(np.uint64)
    g["obs_xy"] = np.arange(2 * len(g["obs_cam"]), dtype=float).reshape(-1, 2)
    ds.write_tracks_dataset(str(tmp_path), g)
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(str(tmp_path), rec, vg, cov)
    o, p = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    for v in range(6):
        o[v], p[v] = g["rot_aa"][v], g["cam_pos"][v]
    sfm.SetReconstructionFromEstimatedPoses(o, p, rec)
    for t in range(len(TRACKS)):
        rec.SetTrack(t, np.array([float(t), 0.0, 1.0]), t != 8)
    return sfm, rec


def test_two_rounds(tmp_path):
    sfm, rec = _reconstruction(tmp_path)
    assert rec.NumEstimatedTracks() == 8 and sorted(rec.EstimatedPositions().keys()) == list(range(6))
    st = sfm.SetUnderconstrainedAsUnestimated(rec)
    assert st == {"rounds": 3, "views_removed": 2, "tracks_removed": 4}
    assert sorted(rec.EstimatedPositions().keys()) == [0, 1, 2, 3] and sorted(rec.EstimatedOrientations().keys()) == [0, 1, 2, 3]
    assert rec.EstimatedTrackIds() == [0, 1, 2, 3]
    assert list(rec.FlattenedTracks()["cam_estimated"]) == [1, 1, 1, 1, 0, 0]
    assert list(rec.TrackPoint(5)) == [5.0, 0.0, 1.0]            # an unestimated track keeps its point
    again = sfm.SetUnderconstrainedAsUnestimated(rec)             # nothing left to do: one round
    assert again == {"rounds": 1, "views_removed": 0, "tracks_removed": 0} and rec.EstimatedTrackIds() == [0, 1, 2, 3]


def test_a_reconstruction_without_tracks_is_left_alone():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    rec = sfm.Reconstruction()
    rec.SetOrientation(0, np.zeros(3))
    assert sfm.SetUnderconstrainedAsUnestimated(rec) == {"rounds": 0, "views_removed": 0, "tracks_removed": 0}
    assert list(rec.EstimatedOrientations().keys()) == [0]


def test_options_carry_the_iterative_solver_threshold(tmp_path):
    from globalsfmpy_amd import GlobalSfMpy as sfm
    assert sfm.ReconstructionEstimatorOptions().min_cameras_for_iterative_solver == 1000
    flags = tmp_path / "flags.yaml"
    flags.write_text("min_cameras_for_iterative_solver: 7\nbundle_adjustment_robust_loss_function: HUBER\nbundle_adjustment_robust_loss_width: 10.0\n")
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts)
    o = opts.reconstruction_estimator_options
    assert (o.min_cameras_for_iterative_solver, o.bundle_adjustment_loss_function_type, o.bundle_adjustment_robust_loss_width) == (7, "HUBER", 10.0)
