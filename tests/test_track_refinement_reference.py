"""The two restatements of the track refinement (tests/track_refinement_reference.py) against each other and against an independent
minimiser, the yardstick of the device test (tests/golden/track_refinement_spread.json, written by tools/make_track_refinement_golden.py and
held here to a recomputation), and what gsfm_tracks_triangulate_refine answers on a machine without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from globalsfmpy_amd import _abi, solver

import track_refinement_reference as ref
import triangulation_reference as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "track_refinement_spread.json")
COS, MAX_SQ = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2


@pytest.fixture(scope="module")
def batch():
    return ref.make_batch()


@pytest.fixture(scope="module")
def recomputed(batch):
    return ref.compute_golden(batch)


def test_batch_holds_the_hand_placed_tracks(batch, recomputed):
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    assert batch["n_base"] == 397 and len(lengths) == 397 + len(ref.HAND_PLACED)
    hand = {k: recomputed["cases"][ref.hand_index(batch, k)] for k in ref.HAND_PLACED}
    assert [hand[k]["length"] for k in ref.HAND_PLACED] == [7, 8, 5, 2, 5, 8, 9, 64, 65, 130]
    assert all(hand[k]["status"] == 0 for k in ref.HAND_PLACED)
    assert hand["unestimated_in_the_middle"]["n_views"] == 4 and hand["two_views"]["n_views"] == 2
    sl = tri.track_slices(batch)
    # the midpoint fails the 15 px gate, the refined point passes it, neither by a hair
    t = ref.hand_index(batch, "midpoint_fails_the_gate_refined_passes")
    mid = ref.refine_mp(batch, *sl[t], COS, MAX_SQ, refine=False)
    assert mid.status == 5 and float(mid.mean_sq_err) > 1.2 * MAX_SQ and hand["midpoint_fails_the_gate_refined_passes"]["mean_sq_err"] < 0.5 * MAX_SQ
    # one observation 30 px off: Huber and Trivial give different points, both estimated
    t = ref.hand_index(batch, "one_outlier_observation")
    a, b = ref.refine_mp(batch, *sl[t], COS, MAX_SQ, loss=ref.TRIVIAL), ref.refine_mp(batch, *sl[t], COS, MAX_SQ, loss=ref.HUBER10)
    assert a.status == b.status == 0 and np.linalg.norm(a.point - b.point) > 1e-3
    assert 0 < hand["noise_free"]["iterations"] <= 2 and hand["noise_free"]["final_cost"] < 1e-15
    # the random part brings slow tracks: a fast and a slow one can share a wavefront
    its = [cs["iterations"] for cs in recomputed["cases"][:batch["n_base"]]]
    assert max(its) >= 40 and sorted(its)[len(its) // 2] <= 3


def test_unrefined_restatement_is_the_triangulation_restatement(batch):
    for t, (oc, xy) in enumerate(tri.track_slices(batch)[:60]):
        a, b = ref.refine_fp64(batch, oc, xy, COS, MAX_SQ, refine=False), tri.triangulate_fp64(batch, oc, xy, COS, MAX_SQ)
        assert a.status == b.status and a.n_views == b.n_views, t
        if a.status in (0, 4, 5):     # the same formulas, evaluated scalar by scalar here and through numpy's products there: rounding apart
            assert tri.relative_deviation(a.point, b.point, tri.origin_centroid(batch, oc)) < 1e-11, t      # the bound test_triangulation_reference puts on the spread
            assert abs(float(a.mean_sq_err) - float(b.mean_sq_err)) <= 1e-9 * max(1.0, float(b.mean_sq_err)), t


def test_numpy_restatement_agrees_with_mpmath_outside_the_flagged_tracks(batch, recomputed):
    cases = recomputed["cases"]
    flagged = [t for t, cs in enumerate(cases) if cs["near"]]
    print("flagged (a decision within %.0e of its threshold): %d of %d tracks; spread_max %.3e" % (ref.NEAR_REL, len(flagged), len(cases), recomputed["spread_max"]))
    assert len(flagged) == recomputed["num_near"] and len(flagged) <= ref.MAX_FLAGGED_FRACTION * len(cases)
    for t, cs in enumerate(cases):
        if t not in flagged:
            assert all(cs["fp64_agrees"]), (t, cs["status"], cs["termination"], cs["iterations"], cs["fp64_agrees"])
    # the header's order, which the 8 sequential orders do not sample
    sl = tri.track_slices(batch)
    for t, cs in enumerate(cases):
        if t in flagged or (t % 4 and t < batch["n_base"]):
            continue
        lane = ref.refine_fp64(batch, *sl[t], COS, MAX_SQ, order="lane")
        assert (lane.status, lane.termination, lane.iterations) == (cs["status"], cs["termination"], cs["iterations"]), t
    assert 0 < recomputed["spread_max"] < 1e-9
    assert {cs["termination"] for cs in cases} >= {-1, ref.FUNCTION_TOLERANCE, ref.GRADIENT_TOLERANCE, ref.PARAMETER_TOLERANCE, ref.NO_CONVERGENCE}


def test_final_cost_never_exceeds_the_initial_cost(recomputed):
    n = 0
    for t, cs in enumerate(recomputed["cases"]):
        if cs["termination"] >= 0:
            assert cs["final_cost"] <= cs["initial_cost"], t
            n += 1
    assert n >= 350


def test_minimiser_agrees_with_scipy_on_trivial_loss_tracks(batch):
    optimize = pytest.importorskip("scipy.optimize")
    sl = tri.track_slices(batch)
    picks = [ref.hand_index(batch, k) for k in ref.HAND_PLACED] + list(range(0, batch["n_base"], 25))
    n = 0
    for t in picks:
        oc, xy = sl[t]
        r = ref.refine_fp64(batch, oc, xy, COS, MAX_SQ, loss=ref.TRIVIAL, options={"function_tolerance": 1e-14, "max_num_iterations": 200})
        if r.termination < 0 or r.termination == ref.NO_CONVERGENCE:
            continue
        keep = [k for k in range(len(oc)) if batch["estimated"][oc[k]]]
        R = [tri.rotation_matrix(batch["rot_aa"][oc[k]]) for k in keep]

        def residuals(X):
            out = []
            for Rk, k in zip(R, keep):
                p = Rk @ (X - batch["cam_pos"][oc[k]])
                f, u, v = batch["intrinsics"][oc[k]]
                out += [f * p[0] / p[2] + u - xy[k][0], f * p[1] / p[2] + v - xy[k][1]]
            return np.array(out)
        sol = optimize.least_squares(residuals, r.point, xtol=1e-15, ftol=1e-15, gtol=1e-15)
        # (1e-15 px^2: a cost that is the rounding of the pixels -- the noise-free track's 1e-19 -- is no quantity to agree on)
        assert abs(sol.cost - float(r.final_cost)) <= 1e-9 * sol.cost + 1e-15, (t, sol.cost, float(r.final_cost))
        assert np.linalg.norm(sol.x - r.point) <= 1e-5 * max(1.0, np.linalg.norm(r.point)), t
        n += 1
    assert n >= 20


def test_golden_file_matches_a_recomputation(recomputed):
    with open(GOLDEN) as f:
        got = json.load(f)
    for k in ("hand_seed", "batch_seed", "orders", "mp_dps", "loss", "min_angle_degrees", "max_error_pixels", "num_near"):
        assert got[k] == recomputed[k], k
    assert len(got["cases"]) == len(recomputed["cases"])
    for t, (a, b) in enumerate(zip(got["cases"], recomputed["cases"])):
        for k in ("length", "status", "n_views", "iterations", "termination", "near"):
            assert a[k] == b[k], (t, k, a[k], b[k])
        pa, pb = np.array([float.fromhex(x) for x in a["point"]]), np.array([float.fromhex(x) for x in b["point"]])
        assert np.max(np.abs(pa - pb)) <= 4 * 2.0 ** -53 * max(1.0, np.max(np.abs(pb))), t      # the same 50-digit value, rounded
        assert abs(a["final_cost"] - b["final_cost"]) <= 4 * 2.0 ** -53 * abs(b["final_cost"]), t
    assert got["spread_max"] == max(cs["spread"] for cs in got["cases"])
    assert 0.25 * recomputed["spread_max"] <= got["spread_max"] <= 4.0 * recomputed["spread_max"]   # rounding errors: another libm reorders them


# ---- the C entry point on a machine without a device ----
def _call_args(b, options=None, loss=((_abi.LOSS_HUBER, 10.0),)):
    dp, u32, i32, u64 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    T = len(b["track_ptr"]) - 1
    out = {"points": np.zeros((T, 3)), "status": np.zeros(T, dtype=np.int32)}
    prog, n = _abi.make_program(list(loss))
    args = [b["n_cams"], b["rot_aa"].ctypes.data_as(dp), b["cam_pos"].ctypes.data_as(dp), b["intrinsics"].ctypes.data_as(dp), None, T,
            b["track_ptr"].ctypes.data_as(u64), b["obs_cam"].ctypes.data_as(u32), b["obs_xy"].ctypes.data_as(dp), 4.0, 15.0,
            None if options is None else C.byref(options), prog, n,
            out["points"].ctypes.data_as(dp), out["status"].ctypes.data_as(i32), None, None, None, None, None, None, None, None]
    return args, out


def _defaults():
    o = _abi.TrackRefineOptions()
    _abi.load_library().gsfm_tracks_refine_default_options(C.byref(o))
    return o


def test_symbol_is_exported_and_declared():
    lib = _abi.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsfm_tracks.h")).read(), flags=re.S)
    m = re.search(r"gsfm_status\s+gsfm_tracks_triangulate_refine\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m and hasattr(lib, "gsfm_tracks_triangulate_refine")
    assert len(lib.gsfm_tracks_triangulate_refine.argtypes) == len([x for x in m.group(1).split(",") if x.strip()]) == 24
    o = _defaults()
    assert (o.refine, o.max_num_iterations, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease,
            o.initial_trust_region_radius, o.max_trust_region_radius, o.min_trust_region_radius) == (1, 100, 1e-6, 1e-10, 1e-8, 1e-3, 1e4, 1e12, 1e-32)
    fields = re.search(r"typedef struct \{(.*?)\}\s*gsfm_tracks_refine_options;", hdr, flags=re.S).group(1)
    assert [f.split()[-1] for f in fields.split(";") if f.strip()] == [name for name, _ in _abi.TrackRefineOptions._fields_]


def test_invalid_arguments_are_rejected_before_any_device_call(batch):
    lib = _abi.load_library()
    good, _ = _call_args(batch)
    for k in (1, 2, 3, 6, 7, 8, 14, 15):                 # NULL required pointers
        args = list(good)
        args[k] = None
        assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG, k
    args = list(good)
    args[12] = None                                      # one node announced, none given
    assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG
    for loss in (((_abi.LOSS_MAGSAC, 0.02, 3, 0),), ((_abi.LOSS_CAUCHY, 1.0),), ((_abi.LOSS_HUBER, 1.0), (_abi.LOSS_OP_SCALE, 2.0)),
                 ((_abi.LOSS_HUBER, 0.0),), ((_abi.LOSS_HUBER, float("nan")),), ((99, 1.0),)):
        args, _ = _call_args(batch, loss=loss)
        assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG, loss
    for field, bad in (("function_tolerance", -1.0), ("gradient_tolerance", float("nan")), ("parameter_tolerance", float("inf")),
                       ("initial_trust_region_radius", 0.0), ("max_trust_region_radius", -1.0), ("min_trust_region_radius", float("nan"))):
        o = _defaults()
        setattr(o, field, bad)
        args, _ = _call_args(batch, options=o)
        assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG, field
    cam = batch["obs_cam"].copy()
    cam[17] = batch["n_cams"]
    args = list(good)
    args[7] = cam.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG and b"out-of-range camera" in lib.gsfm_last_error()
    for k in (9, 10):
        args = list(good)
        args[k] = float("nan")
        assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG, k
    with pytest.raises(solver.SolverError, match="MAGSAC"):
        solver.triangulate_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], batch["obs_cam"], batch["obs_xy"],
                                  refine=True, loss=[(_abi.LOSS_MAGSAC, 0.02, 3, 0)])


def test_valid_call_without_a_device_returns_no_device(batch):
    """on a machine with a device the same call succeeds; the device tests look at what it returns"""
    lib = _abi.load_library()
    for options in (None, _defaults()):
        good, out = _call_args(batch, options=options)
        st = lib.gsfm_tracks_triangulate_refine(*good)
        if st == 0:                                       # this machine has a device
            assert set(out["status"]) <= {0, 1, 2, 3, 4, 5, 6} and out["points"].any()
            continue
        assert st == _abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gsfm_last_error()
        assert not out["points"].any()
    args = list(good)
    args[5] = 0                                           # no tracks: nothing to do, with or without a device
    assert lib.gsfm_tracks_triangulate_refine(*args) == 0
