"""CPU: the tracks of the point-to-camera constraints of position estimation (include/gsfm/position_track_selection.hpp).

The header against a Python restatement of the reference's FindTracksForProblem / GetTracksSortedByNumViews with this build's fixed
orders (views ascending; candidates by NumViews descending, then TrackId ascending), through the module's SelectTracksForPositionEstimation,
on cases with ties, a view below the minimum, a view already credited by earlier tracks and tracks with views that have no position; the
weight formula; the stand-alone C++ test, also under AddressSanitizer and UndefinedBehaviorSanitizer; the options and the YAML keys."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


def select(positioned, track_ptr, obs_view, minimum):
    """the restatement: (chosen tracks ascending, credits per positioned view)"""
    T = len(track_ptr) - 1
    views_of = [sorted(set(int(v) for v in obs_view[track_ptr[t]:track_ptr[t + 1]])) for t in range(T)]
    credits = {int(v): 0 for v in positioned}
    chosen = set()
    if minimum <= 0:
        return [], credits
    for v in sorted(credits):
        if sum(int(w) == v for w in obs_view) < minimum:
            continue
        cand = sorted((t for t in range(T) if v in views_of[t] and t not in chosen), key=lambda t: (-len(views_of[t]), t))
        for t in cand:
            if credits[v] >= minimum:
                break
            chosen.add(t)
            for w in views_of[t]:
                if w in credits:
                    credits[w] += 1
    return sorted(chosen), credits


def _check(sfm, positioned, track_ptr, obs_view, minimum):
    got = sfm.SelectTracksForPositionEstimation([int(v) for v in positioned], [int(p) for p in track_ptr], [int(v) for v in obs_view], minimum)
    tracks, credits = select(positioned, track_ptr, obs_view, minimum)
    assert list(got["tracks"]) == tracks and dict(got["credits"]) == credits
    assert got["num_point_to_camera_constraints"] == sum(credits.values())
    return tracks, credits


def test_selection_against_the_restatement():
    sfm = _sfm()
    # ties (tracks 1 and 2, 4 and 5), view 3 credited by earlier tracks, view 9 without a position
    ptr = [0, 2, 5, 8, 11, 13, 15, 18]
    view = [1, 2, 1, 2, 3, 1, 3, 9, 2, 3, 4, 4, 5, 5, 9, 3, 4, 5]
    tracks, credits = _check(sfm, [5, 3, 1, 2, 4], ptr, view, 2)
    assert tracks == [1, 2, 3, 4, 6] and credits == {1: 2, 2: 2, 3: 4, 4: 3, 5: 2}
    # a minimum that only view 3 has the features for: the others are skipped, and credited all the same
    tracks, credits = _check(sfm, [1, 2, 3, 4, 5], ptr, view, 4)
    assert tracks == [1, 2, 3, 6] and credits[3] == 4 and credits[5] == 1
    assert _check(sfm, [1, 2, 3, 4, 5], ptr, view, 0) == ([], {1: 0, 2: 0, 3: 0, 4: 0, 5: 0})
    rng = np.random.default_rng(4)
    for minimum in (1, 2, 5, 9):
        lengths = rng.integers(2, 7, 120)
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        view = rng.integers(0, 30, ptr[-1])
        positioned = [v for v in range(30) if v % 5 != 4]
        tracks, credits = _check(sfm, positioned, ptr, view, minimum)
        assert tracks and any(w not in credits for t in tracks for w in view[ptr[t]:ptr[t + 1]])   # chosen tracks with views that have no position


def test_weight_formula():
    sfm = _sfm()
    assert sfm.PointToCameraWeight(0.5, 300, 533) == 0.5 * 300.0 / 533.0
    assert sfm.PointToCameraWeight(0.25, 8, 2) == 1.0


@pytest.mark.parametrize("sanitize", [False, True])
def test_selection_header_stand_alone(tmp_path, sanitize):
    exe = str(tmp_path / "position_track_selection_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "position_track_selection_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr


def test_options_and_yaml_keys(tmp_path):
    sfm = _sfm()
    o = sfm.NonlinearPositionEstimatorOptions()
    assert (o.min_num_points_per_view, o.point_to_camera_weight, o.rays_from_reconstruction_orientation, o.robust_loss_width, o.max_num_iterations) == \
        (0, 0.5, False, 0.1, 400)
    cfg = tmp_path / "flags.yaml"
    cfg.write_text("num_threads: 2\nposition_estimation_min_num_tracks_per_view: 3\nposition_estimation_robust_loss_width: 0.25\n")
    b = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(cfg), b)
    p = b.reconstruction_estimator_options.nonlinear_position_estimator_options
    assert p.min_num_points_per_view == 3 and p.robust_loss_width == 0.25 and p.point_to_camera_weight == 0.5
    cfg.write_text("num_threads: 2\n")   # absent keys leave the defaults
    b = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(cfg), b)
    assert b.reconstruction_estimator_options.nonlinear_position_estimator_options.min_num_points_per_view == 0
    # the estimator refuses what the reference CHECKs, and point constraints without a reconstruction, before any device call
    o.min_num_points_per_view = 2
    e = sfm.NonlinearPositionEstimator(o)
    vp, ori, pos = sfm.MapEdges(), sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    info = sfm.TwoViewInfo()
    info.position_2 = np.array([1.0, 0.0, 0.0])
    vp[(0, 1)] = info
    ori[0] = np.zeros(3)
    ori[1] = np.zeros(3)
    assert not e.EstimatePositions(vp, ori, pos) and "reconstruction" in e.LastError()
    o.point_to_camera_weight = 0.0
    e = sfm.NonlinearPositionEstimator(o, sfm.Reconstruction())
    assert not e.EstimatePositions(vp, ori, pos) and "point_to_camera_weight" in e.LastError()
    assert e.options.min_num_points_per_view == 2 and e.LastPointConstraints()["num_tracks"] == 0
