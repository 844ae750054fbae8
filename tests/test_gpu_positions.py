"""Camera-position estimation on the device (include/gsfm_pos.h) against the numpy reference (tests/position_reference.py).
Everything runs in the pytest process.  Positions are compared after removing translation and scale (synth.gauge_normalize)."""
import os

import numpy as np
import pytest

from globalsfmpy_amd import synth
from globalsfmpy_amd import loss_functions as lf
from globalsfmpy_amd.solver import PositionProblem

from position_reference import PositionReference

pytestmark = pytest.mark.gpu


def _problem(g, loss):
    p = PositionProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"])
    p.set_loss(loss)
    return p


def _reference(g, loss):
    return PositionReference(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], loss)


def _gauge_err(a, b, fixed=0):
    return np.abs(synth.gauge_normalize(a, fixed) - synth.gauge_normalize(b, fixed)).max()


def _assert_parity(xd, sd, xr, sr, fixed=0):
    assert sd["final_cost"] == pytest.approx(sr["final_cost"], rel=1e-9, abs=1e-300), (sd, sr)
    assert _gauge_err(xd, xr, fixed) <= 1e-6, (_gauge_err(xd, xr, fixed), sd, sr)
    assert sd["termination"] == sr["termination"], (sd, sr)


@pytest.mark.parametrize("n_cams,n_edges,dense", [(50, 400, True), (300, 3000, True), (300, 3000, False), (2000, 20000, False)])
def test_known_answer(n_cams, n_edges, dense):
    g = synth.make_position_graph(n_cams, n_edges, seed=n_cams)
    p = _problem(g, lf.HuberLoss(0.1))
    x, s = p.solve(None, fixed_cam=0, dense_max_cams=(100000 if dense else 0))
    assert (s["num_dense_solves"] > 0) == dense and (s["num_cg_iterations"] > 0) == (not dense), s
    assert s["nonfinite"] == 0 and s["termination"] != 4, s
    assert np.all(x[0] == 0.0)
    assert _gauge_err(x, g["gt_pos"]) <= 1e-8, (_gauge_err(x, g["gt_pos"]), s)


class PyHuber(object):
    """a loss the device only reaches through the host callback (no native_program)"""

    def __init__(self, a):
        self.inner = lf.HuberLoss(a)

    def Evaluate(self, s, out):
        self.inner.Evaluate(s, out)


@pytest.mark.parametrize("loss", [lf.HuberLoss(0.1), lf.SoftLOneLoss(0.1), lf.CauchyLoss(0.1), "callback"])
def test_parity_with_outliers(loss):
    n_cams, n_edges = (60, 500) if loss == "callback" else (200, 2000)
    g = synth.make_position_graph(n_cams, n_edges, seed=11, outlier_frac=0.3, noise=0.01)
    dev_loss = PyHuber(0.1) if loss == "callback" else loss
    ref_loss = lf.HuberLoss(0.1) if loss == "callback" else loss
    xd, sd = _problem(g, dev_loss).solve(None, fixed_cam=0)
    xr, sr = _reference(g, ref_loss).solve(None, fixed_cam=0)
    assert sd["num_dense_solves"] > 0
    _assert_parity(xd, sd, xr, sr)


def test_dense_and_pcg_agree():
    g = synth.make_position_graph(400, 4000, seed=4, outlier_frac=0.3, noise=0.01)
    p = _problem(g, lf.HuberLoss(0.1))
    xd, sd = p.solve(None, fixed_cam=0, dense_max_cams=1000)
    xp, sp = p.solve(None, fixed_cam=0, dense_max_cams=0)
    assert sd["num_dense_solves"] == sd["num_iterations"] and sp["num_dense_solves"] == 0 and sp["num_cg_iterations"] > 0
    assert sp["num_pcg_stalled_steps"] == 0, sp
    _assert_parity(xp, sp, xd, sd)


def test_pcg_path_beyond_5000_cameras():
    # (local topology: the reference's sparse direct solve of a random graph's normal matrix fills in completely)
    g = synth.make_position_graph(5200, 52000, seed=8, outlier_frac=0.3, noise=0.01, local_window=400)
    xd, sd = _problem(g, lf.HuberLoss(0.1)).solve(None, fixed_cam=0)
    # (the local topology's Laplacian is ill-conditioned: a step may end on the stall rule, and the parity below still holds)
    assert sd["num_dense_solves"] == 0 and sd["num_cg_iterations"] > 0 and sd["num_pcg_stalled_steps"] <= 2, sd
    xr, sr = _reference(g, lf.HuberLoss(0.1)).solve(None, fixed_cam=0)
    _assert_parity(xd, sd, xr, sr)


@pytest.mark.parametrize("dense_max_cams", [1000, 0])
def test_deterministic(dense_max_cams):
    g = synth.make_position_graph(600, 8000, seed=21, outlier_frac=0.3, noise=0.01)
    p = _problem(g, lf.HuberLoss(0.1))
    x1, s1 = p.solve(None, fixed_cam=3, dense_max_cams=dense_max_cams)
    x2, s2 = _problem(g, lf.HuberLoss(0.1)).solve(None, fixed_cam=3, dense_max_cams=dense_max_cams)
    assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
    assert s1["final_cost"] == s2["final_cost"] and s1["num_iterations"] == s2["num_iterations"]


def test_one_problem_object_across_solver_paths():
    """PCG, then the dense step (its tiles allocated and cleared at first use, in the stream's order), then a host-callback loss (its
    buffers allocated at first use) on ONE problem object: each solve equals, bit for bit, the same solve on a fresh problem -- nothing a
    solve finds in the problem's memory depends on what ran there before."""
    g = synth.make_position_graph(50, 400, seed=3, outlier_frac=0.2)
    p = _problem(g, lf.HuberLoss(0.1))
    for loss, kw in ((None, {"dense_max_cams": 0}), (None, {"dense_max_cams": 1000}), (PyHuber(0.1), {})):
        if loss is not None:
            p.set_loss(loss)
        x1, s1 = p.solve(None, fixed_cam=0, **kw)
        x2, s2 = _problem(g, loss if loss is not None else lf.HuberLoss(0.1)).solve(None, fixed_cam=0, **kw)
        assert np.array_equal(x1, x2), kw
        assert s1["num_iterations"] == s2["num_iterations"] and s1["termination"] == s2["termination"], (s1, s2)
        assert (s1["num_dense_solves"] > 0) == (kw.get("dense_max_cams") != 0), s1


@pytest.mark.parametrize("dense_max_cams", [1000, 0])
def test_large_radius_scale_gauge(dense_max_cams):
    """The radius grows to >= 1e12, where the damped step system's condition number along the scale direction v = c - c_0 is of the
    order of the radius: with that component projected out of every step, the two exact solvers (dense Cholesky / PCG on the device,
    Cholesky in the reference) still agree on the positions, and the fixed camera does not move."""
    g = synth.make_position_graph(300, 3000, seed=2, outlier_frac=0.1, noise=0.02)
    # (started at radius 1e10 so that a few successful steps take it past 1e12; from 1e4 this graph stops at ~6e8)
    xd, sd = _problem(g, lf.HuberLoss(0.1)).solve(None, fixed_cam=5, dense_max_cams=dense_max_cams, initial_trust_region_radius=1e10)
    xr, sr = _reference(g, lf.HuberLoss(0.1)).solve(None, fixed_cam=5, initial_trust_region_radius=1e10)
    assert sd["max_radius"] >= 1e12 and sr["max_radius"] >= 1e12, (sd, sr)
    assert np.all(xd[5] == 0.0)
    _assert_parity(xd, sd, xr, sr, fixed=5)


def test_residuals_and_untouched_cameras():
    g = synth.make_position_graph(40, 200, seed=1, outlier_frac=0.2, noise=0.05)
    # camera 40 appears in no edge: not a parameter, passes through the solve untouched
    p = PositionProblem(41, g["edge_i"], g["edge_j"], g["rel_t"], np.vstack([g["rot_aa"], [[0.1, 0.2, 0.3]]]))
    p.set_loss(lf.CauchyLoss(0.2))
    init = np.zeros((41, 3))
    init[40] = [7.0, 8.0, 9.0]
    x, s = p.solve(init, fixed_cam=0)
    assert np.array_equal(x[40], [7.0, 8.0, 9.0])
    ref = _reference(g, lf.CauchyLoss(0.2))
    r, rho = p.residuals(x)
    rr = ref.residuals(x[:40])[0]
    np.testing.assert_allclose(r, rr, rtol=0, atol=1e-15)
    s2 = np.sum(rr * rr, axis=1)
    want = np.array([(lambda out: (lf.CauchyLoss(0.2).Evaluate(v, out), out[0])[1])([0.0, 0.0, 0.0]) for v in s2])
    np.testing.assert_allclose(rho, want, rtol=1e-13)
    assert 0.5 * rho.sum() == pytest.approx(s["final_cost"], rel=1e-12)


# ---- the C++ estimator and the pybind module --------------------------------------------------------------------------------------

def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


def _flatten(view_pairs, orientations, positions):
    """the shim's dense numbering: sorted keys of `positions`, the used view pairs in sorted order"""
    ids = sorted(int(k) for k in positions.keys())
    index = {v: k for k, v in enumerate(ids)}
    keys = sorted(k for k in view_pairs.keys() if k[0] in index and k[1] in index and k[0] in orientations)
    ei = np.array([index[k[0]] for k in keys], dtype=np.uint32)
    ej = np.array([index[k[1]] for k in keys], dtype=np.uint32)
    rel = np.array([view_pairs[k].position_2 for k in keys]).reshape(-1, 3)
    rot = np.array([orientations[v] if v in orientations else np.zeros(3) for v in ids])
    return ids, index, ei, ej, rel, rot


def test_estimator_shim_rules_and_fixed_view():
    sfm = _sfm()
    g = synth.make_position_graph(80, 600, seed=9, outlier_frac=0.2, noise=0.01)
    ids = np.arange(80) * 5 + 2   # sparse ViewIds
    vg = sfm.ViewGraph()
    for i, j, t in zip(g["edge_i"], g["edge_j"], g["rel_t"]):
        info = sfm.TwoViewInfo()
        info.position_2 = t
        vg.AddEdge(int(ids[i]), int(ids[j]), info)
    lone = sfm.TwoViewInfo()
    lone.position_2 = np.array([1.0, 0.0, 0.0])
    vg.AddEdge(int(ids[0]), 1001, lone)        # view 1001 has no orientation: no position, the edge is skipped
    o = sfm.MapViewIdVector3d()
    for k in range(80):
        o[int(ids[k])] = g["rot_aa"][k]
    o[2000] = np.array([0.1, 0.2, 0.3])        # an orientation without a view pair: no position
    positions = sfm.MapViewIdVector3d()
    est = sfm.NonlinearPositionEstimator()
    assert est.EstimatePositions(vg.GetAllEdges(), o, positions), est.LastError()
    assert sorted(int(k) for k in positions.keys()) == sorted(int(v) for v in ids)
    fixed = est.FixedView()
    assert fixed == next(iter(positions.keys()))          # positions->begin(), as the reference holds it
    assert np.all(np.asarray(positions[fixed]) == 0.0)
    s = est.LastSummary()
    assert s["num_edges_used"] == 600 and s["termination"] != 4
    vids, index, ei, ej, rel, rot = _flatten(vg.GetAllEdges(), o, positions)
    flat = PositionProblem(len(vids), ei, ej, rel, rot)
    flat.set_loss(lf.HuberLoss(0.1))                      # the overload without a loss: HuberLoss(robust_loss_width = 0.1)
    xf, sf = flat.solve(None, fixed_cam=index[int(fixed)])
    xd = np.array([positions[v] for v in vids])
    assert np.array_equal(xd, xf) and sf["final_cost"] == s["final_cost"]
    # an explicit loss goes to the device as its program; the error type is accepted and has no effect
    positions2 = sfm.MapViewIdVector3d()
    assert est.EstimatePositions(vg.GetAllEdges(), o, positions2, lf.CauchyLoss(0.1), sfm.PositionErrorType.BASELINE)
    flat.set_loss(lf.CauchyLoss(0.1))
    xf2, sf2 = flat.solve(None, fixed_cam=index[int(est.FixedView())])
    assert np.array_equal(np.array([positions2[v] for v in vids]), xf2)


def test_1dsfm_sample_pipeline(golden_dir):
    """Read1DSFM -> FilterInitialViewGraphAndCalibrateCameras -> EstimateGlobalRotations(HuberLoss(0.1)) -> FilterRotations ->
    NonlinearPositionEstimator.EstimatePositions on the fixture's real position_2 values, against the reference run on the same
    rotations with the same fixed camera."""
    import os
    sfm = _sfm()
    rec, vg, cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(os.path.join(golden_dir, "1dsfm_sample"), rec, vg, cov)
    est = sfm.GlobalReconstructionEstimator(sfm.ReconstructionBuilderOptions().reconstruction_estimator_options)
    assert est.FilterInitialViewGraphAndCalibrateCameras(vg, rec)
    assert est.EstimateGlobalRotations(lf.HuberLoss(0.1))
    est.FilterRotations()
    positions = sfm.MapViewIdVector3d()
    pe = sfm.NonlinearPositionEstimator()
    assert pe.EstimatePositions(vg.GetAllEdges(), est.orientations, positions, lf.HuberLoss(0.1)), pe.LastError()
    vids, index, ei, ej, rel, rot = _flatten(vg.GetAllEdges(), est.orientations, positions)
    assert len(vids) >= 20 and np.abs(rel).max() > 0
    fixed = index[int(pe.FixedView())]
    xr, sr = PositionReference(len(vids), ei, ej, rel, rot, lf.HuberLoss(0.1)).solve(None, fixed_cam=fixed)
    xd = np.array([positions[v] for v in vids])
    _assert_parity(xd, pe.LastSummary(), xr, sr, fixed=fixed)


def test_ply_writes_estimated_positions(tmp_path):
    sfm = _sfm()
    g = synth.make_position_graph(30, 150, seed=6)
    vg = sfm.ViewGraph()
    for i, j, t in zip(g["edge_i"], g["edge_j"], g["rel_t"]):
        info = sfm.TwoViewInfo()
        info.position_2 = t
        vg.AddEdge(int(i), int(j), info)
    o = sfm.MapViewIdVector3d()
    for k in range(30):
        o[k] = g["rot_aa"][k]
    positions = sfm.MapViewIdVector3d()
    assert sfm.NonlinearPositionEstimator().EstimatePositions(vg.GetAllEdges(), o, positions)
    rec = sfm.Reconstruction()
    for k in range(31):               # view 30 has no estimate: not written
        rec.SetViewName(k, "v%d" % k)
    sfm.SetReconstructionFromEstimatedPoses(o, positions, rec)
    assert len(rec.EstimatedPositions()) == 30
    path = tmp_path / "positions.ply"
    assert sfm.WritePlyFile(str(path), rec, 2)
    lines = path.read_text().splitlines()
    assert lines[2] == "element vertex 30" and lines[9] == "end_header"
    verts = np.array([[float(v) for v in line.split()] for line in lines[10:]])
    assert verts.shape == (30, 6) and np.all(verts[:, 3:] == [0, 255, 0])
    want = np.array([positions[k] for k in range(30)])
    got = sorted(map(tuple, verts[:, :3]))
    np.testing.assert_allclose(np.array(got), np.array(sorted(map(tuple, want))), rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert np.abs(want).max() > 0.1   # the cameras are no longer all at the origin


@pytest.mark.parametrize("tag,options", [("dense", {}), ("pcg", {"dense_max_cams": 0})])
def test_solve_keeps_the_bytes_of_the_commit_before_the_shared_host_loop(tag, options):
    """gsfm_pos_solve under Huber 0.1 from the fixture's start array, by Cholesky steps and by PCG steps: the bytes and counts recorded on an
    MI355X from a library built from the commit before the solvers' host loops moved to csrc/lm_loop.hpp (tools/make_lm_loop_golden.py,
    tests/golden/pos_solve_parent_bytes.npz)."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pos_solve_parent_bytes.npz"))
    g = synth.make_position_graph(60, 500, seed=11, outlier_frac=0.3, noise=0.01)
    x, s = _problem(g, lf.HuberLoss(0.1)).solve(gold["start"], fixed_cam=0, **options)
    counts = [s[k] for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_cg_iterations", "num_dense_solves")]
    print(tag, counts, "final cost %.17g" % s["final_cost"])
    assert (s["num_dense_solves"] > 0) == (tag == "dense") and (s["num_cg_iterations"] > 0) == (tag == "pcg")
    assert x.tobytes() == gold[tag + "_pos"].tobytes()
    assert s["final_cost"] == gold[tag + "_final_cost"][0]
    assert counts == list(gold[tag + "_counts"])
