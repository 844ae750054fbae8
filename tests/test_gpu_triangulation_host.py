"""The host layer of the track triangulation on a synthetic 1DSfM dataset: after SetReconstructionFromEstimatedPoses,
GlobalReconstructionEstimator.EstimateStructure() stores for every track exactly what the flat-array call returns on the arrays
Reconstruction.FlattenedTracks() shows, without per-track refinement whatever bundle_adjust_tracks says; WritePlyFile lists the estimated
tracks before the cameras; a dataset without tracks.txt is left alone."""
import os
import shutil
import sys

import numpy as np
import pytest

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import synth
from globalsfmpy_amd.solver import triangulate_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives, as the reference's scripts append ../build

pytestmark = pytest.mark.gpu

HEADER = "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n" \
         "property uchar green\nproperty uchar blue\nend_header\n"
UNESTIMATED_VIEW = 11


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


@pytest.fixture(scope="module")
def scene():
    return synth.make_tracks(12, 60, 21, lengths=(2, 3, 4, 5, 8, 12), noise_px=0.5, outlier_frac=0.03)


@pytest.fixture(scope="module")
def dataset(scene, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("synthetic_1dsfm_tracks"))
    ds.write_tracks_dataset(path, scene)
    return path


def estimator_with_ground_truth_poses(sfm, path, scene):
    """the pipeline's calls up to SetReconstructionFromEstimatedPoses, with the generator's poses in place of the estimated ones"""
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(path, rec, vg, cov)
    opts = sfm.ReconstructionEstimatorOptions()
    opts.min_num_two_view_inliers = 1              # 60 tracks: a view pair shares a handful
    est = sfm.GlobalReconstructionEstimator(opts)
    assert est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    o, p = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    for v in range(scene["n_cams"]):
        if v != UNESTIMATED_VIEW:
            o[v], p[v] = scene["rot_aa"][v], scene["cam_pos"][v]
    sfm.SetReconstructionFromEstimatedPoses(o, p, rec)
    return est, rec, vg


def ply_lines(path, n_header=10):
    text = open(path).read()
    lines = text.split("\n")
    assert lines[-1] == ""
    return "\n".join(lines[:n_header]) + "\n", lines[n_header:-1]


def camera_lines(rec):
    return sorted("%g %g %g 0 255 0" % tuple(p) for p in rec.EstimatedPositions().values())


def test_estimate_structure_stores_what_the_flat_call_returns(dataset, scene):
    sfm = _sfm()
    est, rec, vg = estimator_with_ground_truth_poses(sfm, dataset, scene)
    T = len(scene["track_ptr"]) - 1
    assert rec.NumTracks() == T and rec.NumEstimatedTracks() == 0 and not rec.TrackIsEstimated(0)
    flat = rec.FlattenedTracks()
    assert list(flat["views"]) == list(range(12)) and list(flat["cam_estimated"]) == [1] * 11 + [0]
    assert np.array_equal(flat["track_ptr"], scene["track_ptr"]) and np.array_equal(flat["obs_cam"], scene["obs_cam"])
    assert np.array_equal(flat["obs_xy"], scene["obs_xy"]) and np.array_equal(flat["intrinsics"], scene["intrinsics"])
    assert np.array_equal(flat["rot_aa"][:11], scene["rot_aa"][:11]) and not flat["rot_aa"][11].any()
    assert est.options.bundle_adjust_tracks is True and est.options.min_triangulation_angle_degrees == 4.0
    assert est.options.triangulation_max_reprojection_error_in_pixels == 15.0
    ref = triangulate_tracks(flat["rot_aa"], flat["cam_pos"], flat["intrinsics"], flat["track_ptr"], flat["obs_cam"], flat["obs_xy"],
                             cam_estimated=flat["cam_estimated"], min_triangulation_angle_degrees=4.0, max_reprojection_error_pixels=15.0)
    stats = est.EstimateStructure()
    n_est = int(np.sum(ref["status"] == 0))
    print("EstimateStructure: %s" % stats)
    assert 30 <= n_est < T                       # the outliers and the unestimated view cost some tracks
    assert stats["num_tracks"] == T and stats["num_estimated"] == n_est == rec.NumEstimatedTracks() and stats["kernel_ms"] > 0
    assert list(stats["counts"]) == [int(c) for c in ref["counts"]]
    assert stats["tracks_refined"] is False and stats["bundle_adjust_tracks_requested"] is True and "without per-track refinement" in stats["note"]
    assert est.LastStructureSummary() == stats
    for t in range(T):
        assert rec.TrackIsEstimated(t) == (ref["status"][t] == 0), t
        assert np.array_equal(np.array(rec.TrackPoint(t)).view(np.uint64), ref["points"][t].view(np.uint64)), t
        assert rec.TrackNumViews(t) == int(scene["track_ptr"][t + 1] - scene["track_ptr"][t])
    assert rec.EstimatedTrackIds() == [t for t in range(T) if ref["status"][t] == 0]
    good = np.flatnonzero(ref["status"] == 0)
    assert np.max(np.linalg.norm(ref["points"][good] - scene["gt_points"][good], axis=1)) < 0.2    # 0.5 px noise at 10 units
    with pytest.raises(IndexError):
        rec.TrackPoint(T)
    # the option is read from the YAML and changes nothing
    est.options.bundle_adjust_tracks = False
    again = est.EstimateStructure()
    assert again["bundle_adjust_tracks_requested"] is False and again["counts"] == stats["counts"] and again["tracks_refined"] is False
    assert all(np.array_equal(np.array(rec.TrackPoint(t)).view(np.uint64), ref["points"][t].view(np.uint64)) for t in range(T))


def test_ply_lists_the_estimated_tracks_then_the_cameras(dataset, scene, tmp_path):
    sfm = _sfm()
    est, rec, vg = estimator_with_ground_truth_poses(sfm, dataset, scene)
    before = tmp_path / "before.ply"
    assert sfm.WritePlyFile(str(before), rec, 2)
    head, body = ply_lines(str(before))
    assert head == HEADER % 11 and sorted(body) == camera_lines(rec)       # no estimated track: the cameras alone, as before
    est.EstimateStructure()
    lengths = np.diff(scene["track_ptr"].astype(np.int64))
    for min_obs in (2, 4):
        path = tmp_path / ("after%d.ply" % min_obs)
        assert sfm.WritePlyFile(str(path), rec, min_obs)
        want = ["%g %g %g 0 0 0" % tuple(rec.TrackPoint(t)) for t in rec.EstimatedTrackIds() if lengths[t] >= min_obs]
        head, body = ply_lines(str(path))
        assert len(want) > 5 and head == HEADER % (len(want) + 11)
        assert body[:len(want)] == want and sorted(body[len(want):]) == camera_lines(rec)
    assert len([t for t in rec.EstimatedTrackIds() if lengths[t] < 4]) > 0


def test_yaml_keys_are_read(tmp_path):
    sfm = _sfm()
    flags = tmp_path / "flags.yaml"
    flags.write_text("min_triangulation_angle_degrees: 2.5\ntriangulation_reprojection_error_pixels: 9.0\nbundle_adjust_tracks: false\n")
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts)
    o = opts.reconstruction_estimator_options
    assert o.min_triangulation_angle_degrees == 2.5 and o.triangulation_max_reprojection_error_in_pixels == 9.0 and o.bundle_adjust_tracks is False


def test_dataset_without_tracks_is_left_alone(dataset, scene, tmp_path):
    sfm = _sfm()
    bare = tmp_path / "bare"
    bare.mkdir()
    for name in ("EGs.txt", "cc.txt"):
        shutil.copy(os.path.join(dataset, name), str(bare / name))
    est, rec, vg = estimator_with_ground_truth_poses(sfm, str(bare), scene)
    assert rec.NumTracks() == 0 and rec.FlattenedTracks() is None
    stats = est.EstimateStructure()
    assert stats["num_tracks"] == 0 and stats["num_estimated"] == 0 and stats["kernel_ms"] == 0.0 and rec.NumEstimatedTracks() == 0
    path = tmp_path / "bare.ply"
    assert sfm.WritePlyFile(str(path), rec, 2)
    head, body = ply_lines(str(path))
    assert head == HEADER % 11 and sorted(body) == camera_lines(rec) and all(line.endswith(" 0 255 0") for line in body)
