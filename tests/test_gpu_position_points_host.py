"""-m gpu: the estimator layer of position estimation with point-to-camera constraints on a small synthetic reconstruction (20 views, a
1DSfM dataset written from synth.make_position_scene): NonlinearPositionEstimator(options, reconstruction).EstimatePositions with
min_num_points_per_view = 3 against the flat call (solver.PointPositionProblem) fed with the selection built by hand in Python; the zero
value; the YAML key through GlobalReconstructionEstimator.PositionEstimator(); the ray orientation switch."""
import os
import sys

import numpy as np
import pytest

from globalsfmpy_amd import dataset_1dsfm as ds
from globalsfmpy_amd import loss_functions as lf
from globalsfmpy_amd import synth
from globalsfmpy_amd.solver import PointPositionProblem, PositionProblem

from test_position_track_selection import select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives

pytestmark = pytest.mark.gpu
N_VIEWS, NO_POSITION = 20, 19   # view 19 is in tracks and in no view pair: it gets no position


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


@pytest.fixture(scope="module")
def scene():
    g = synth.make_position_scene(N_VIEWS, 90, 60, seed=7, lengths=(2, 3, 4, 6), noise=0.005, outlier_frac=0.1)
    g["cam_pos"] = g["gt_pos"]
    return g


@pytest.fixture(scope="module")
def world(scene, tmp_path_factory):
    """(sfm, reconstruction with the scene's tracks, view pairs without view 19, orientations)"""
    sfm = _sfm()
    path = str(tmp_path_factory.mktemp("synthetic_position_scene"))
    ds.write_tracks_dataset(path, scene)
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(path, rec, vg, cov)
    assert rec.NumTracks() == 60
    pairs = sfm.ViewGraph()
    for i, j, t in zip(scene["edge_i"], scene["edge_j"], scene["rel_t"]):
        if NO_POSITION in (int(i), int(j)):
            continue
        info = sfm.TwoViewInfo()
        info.position_2 = t
        pairs.AddEdge(int(i), int(j), info)
    o = sfm.MapViewIdVector3d()
    for k in range(N_VIEWS):
        o[k] = scene["rot_aa"][k]
    return sfm, rec, pairs, o, vg


def _flatten(view_pairs, orientations, positions):
    """the shim's dense numbering (tests/test_gpu_positions.py): sorted keys of `positions`, the used view pairs in sorted order"""
    ids = sorted(int(k) for k in positions.keys())
    index = {v: k for k, v in enumerate(ids)}
    keys = sorted(k for k in view_pairs.keys() if k[0] in index and k[1] in index and k[0] in orientations)
    ei = np.array([index[k[0]] for k in keys], dtype=np.uint32)
    ej = np.array([index[k[1]] for k in keys], dtype=np.uint32)
    rel = np.array([view_pairs[k].position_2 for k in keys]).reshape(-1, 3)
    rot = np.array([orientations[v] if v in orientations else np.zeros(3) for v in ids])
    return ids, index, ei, ej, rel, rot


def _by_hand(rec, ids, index, minimum, n_edges, weight=0.5):
    """the arrays the estimator hands down, from Reconstruction.FlattenedTracks() and the Python restatement of the selection"""
    flat = rec.FlattenedTracks()
    obs_view = flat["views"][flat["obs_cam"]]
    tp = flat["track_ptr"].astype(np.int64)
    tracks, credits = select(ids, tp, obs_view, minimum)
    ptr, cam, xy, dropped = [0], [], [], 0
    for t in tracks:
        for e in range(tp[t], tp[t + 1]):
            if int(obs_view[e]) in index:
                cam.append(index[int(obs_view[e])])
                xy.append(flat["obs_xy"][e])
            else:
                dropped += 1   # an observation in a view without a position
        ptr.append(len(cam))
    K = np.zeros((len(ids), 3))
    for c, v in enumerate(flat["views"]):
        if int(v) in index:
            K[index[int(v)]] = flat["intrinsics"][c]
    n_constraints = sum(credits.values())
    return dict(track_ptr=np.array(ptr, np.uint64), obs_cam=np.array(cam, np.uint32), obs_xy=np.array(xy).reshape(-1, 2), intrinsics=K,
                weight=weight * n_edges / n_constraints, num_tracks=len(tracks), num_constraints=n_constraints, dropped=dropped)


def test_estimate_positions_with_point_constraints_equals_the_flat_call(world):
    sfm, rec, pairs, o, _ = world
    opt = sfm.NonlinearPositionEstimatorOptions()
    opt.min_num_points_per_view = 3
    est = sfm.NonlinearPositionEstimator(opt, rec)
    positions = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(pairs.GetAllEdges(), o, positions), est.LastError()   # (before this solver: false, "not implemented")
    ids, index, ei, ej, rel, rot = _flatten(pairs.GetAllEdges(), o, positions)
    assert ids == list(range(N_VIEWS - 1))
    hand = _by_hand(rec, ids, index, 3, len(ei))
    pc, s = est.LastPointConstraints(), est.LastSummary()
    assert (pc["num_tracks"], pc["num_constraints"], pc["weight"]) == (hand["num_tracks"], hand["num_constraints"], hand["weight"])
    assert hand["num_tracks"] >= 10 and pc["num_active_points"] >= 10 and pc["num_observations_used"] <= len(hand["obs_cam"])
    assert hand["dropped"] >= 1   # chosen tracks see the view without a position: those observations are left out
    fixed = est.FixedView()
    flat = PointPositionProblem(len(ids), ei, ej, rel, rot, rot, hand["intrinsics"], hand["track_ptr"], hand["obs_cam"], hand["obs_xy"], hand["weight"])
    flat.set_loss(lf.HuberLoss(0.1))
    xf, pf, sf = flat.solve(fixed_cam=index[int(fixed)])   # cameras at 0, points at (1, 1, 1)
    xd = np.array([positions[v] for v in ids])
    assert np.array_equal(xd, xf) and sf["final_cost"] == s["final_cost"] and sf["num_iterations"] == s["num_iterations"]
    assert sf["num_observations_used"] == pc["num_observations_used"] and sf["num_active_points"] == pc["num_active_points"]
    assert s["termination"] != 4 and np.all(xd[index[int(fixed)]] == 0.0)
    # an explicit native loss reaches both residual kinds; a loss without a native program is refused on a problem with tracks
    positions2 = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(pairs.GetAllEdges(), o, positions2, lf.CauchyLoss(0.1), sfm.PositionErrorType.BASELINE)
    flat.set_loss(lf.CauchyLoss(0.1))
    xf2, _, _ = flat.solve(fixed_cam=index[int(est.FixedView())])
    assert np.array_equal(np.array([positions2[v] for v in ids]), xf2) and not np.array_equal(xf2, xf)

    class PyLoss(sfm.LossFunction):
        def Evaluate(self, s, out):
            out[0], out[1], out[2] = s, 1.0, 0.0

    assert not est.EstimatePositions(pairs.GetAllEdges(), o, sfm.MapViewIdVector3d(), PyLoss(), sfm.PositionErrorType.BASELINE)
    assert "native program" in est.LastError()


def test_the_zero_value_is_the_camera_only_solve(world):
    sfm, rec, pairs, o, _ = world
    plain, with_rec = sfm.NonlinearPositionEstimator(), sfm.NonlinearPositionEstimator(sfm.NonlinearPositionEstimatorOptions(), rec)
    pa, pb = sfm.MapViewIdVector3d(), sfm.MapViewIdVector3d()
    assert plain.EstimatePositions(pairs.GetAllEdges(), o, pa) and with_rec.EstimatePositions(pairs.GetAllEdges(), o, pb)
    ids, index, ei, ej, rel, rot = _flatten(pairs.GetAllEdges(), o, pa)
    flat = PositionProblem(len(ids), ei, ej, rel, rot)
    flat.set_loss(lf.HuberLoss(0.1))
    xf, sf = flat.solve(None, fixed_cam=index[int(plain.FixedView())])
    for p, e in ((pa, plain), (pb, with_rec)):
        assert np.array([p[v] for v in ids]).tobytes() == xf.tobytes() and e.LastSummary()["final_cost"] == sf["final_cost"]
        assert e.LastPointConstraints()["num_tracks"] == 0 and e.LastSummary()["num_dense_solves"] > 0   # gsfm_pos_solve's dense path, as before
    # a minimum no view has the features for chooses nothing: the camera-only solve again
    opt = sfm.NonlinearPositionEstimatorOptions()
    opt.min_num_points_per_view = 1000
    none = sfm.NonlinearPositionEstimator(opt, rec)
    pc = sfm.MapViewIdVector3d()
    assert none.EstimatePositions(pairs.GetAllEdges(), o, pc) and np.array([pc[v] for v in ids]).tobytes() == xf.tobytes()


def test_yaml_key_reaches_the_estimator_and_the_ray_switch(world, tmp_path):
    sfm, rec, pairs, o, vg = world
    cfg = tmp_path / "flags.yaml"
    cfg.write_text("num_threads: 1\nposition_estimation_min_num_tracks_per_view: 3\nposition_estimation_robust_loss_width: 0.1\n")
    b = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(cfg), b)
    b.reconstruction_estimator_options.min_num_two_view_inliers = 1
    gre = sfm.GlobalReconstructionEstimator(b.reconstruction_estimator_options)
    assert gre.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    est = gre.PositionEstimator()   # the estimator's options and its reconstruction handed over
    assert est.options.min_num_points_per_view == 3 and est.options.rays_from_reconstruction_orientation is False
    pa = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(pairs.GetAllEdges(), o, pa), est.LastError()
    ref = sfm.NonlinearPositionEstimator(est.options, rec)
    pb = sfm.MapViewIdVector3d()
    assert ref.EstimatePositions(pairs.GetAllEdges(), o, pb)
    ids = sorted(int(k) for k in pa.keys())
    xa = np.array([pa[v] for v in ids])
    assert xa.tobytes() == np.array([pb[v] for v in ids]).tobytes() and est.LastPointConstraints()["num_tracks"] >= 10
    # rays_from_reconstruction_orientation: the rays are rotated by what the reconstruction stores (the reference's literal behaviour).
    # Nothing stored: identity rotations, another problem; the passed orientations stored: the default's bytes.
    est.options.rays_from_reconstruction_orientation = True
    assert not rec.EstimatedOrientations()
    pc = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(pairs.GetAllEdges(), o, pc), est.LastError()
    _, index, ei, ej, rel, rot = _flatten(pairs.GetAllEdges(), o, pc)
    hand = _by_hand(rec, ids, index, 3, len(ei))
    flat = PointPositionProblem(len(ids), ei, ej, rel, rot, np.zeros_like(rot), hand["intrinsics"], hand["track_ptr"], hand["obs_cam"], hand["obs_xy"], hand["weight"])
    flat.set_loss(lf.HuberLoss(0.1))
    xz, _, _ = flat.solve(fixed_cam=index[int(est.FixedView())])
    xc = np.array([pc[v] for v in ids])
    assert xc.tobytes() == xz.tobytes() and not np.array_equal(xc, xa)
    sfm.SetOrientations(o, rec)
    pd = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(pairs.GetAllEdges(), o, pd)
    assert np.array([pd[v] for v in ids]).tobytes() == xa.tobytes()
