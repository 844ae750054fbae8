"""The two restatements of the outlier rule (tests/outlier_reference.py) against each other, the yardstick of the device test
(tests/golden/outlier_tracks.json, held here to a recomputation), the hand-placed cases, and what gsfm_tracks_outlier_tracks answers on a
machine without a device."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from globalsfmpy_amd import _abi, solver

import outlier_reference as out
import triangulation_reference as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "outlier_tracks.json")


@pytest.fixture(scope="module")
def batch():
    return out.make_batch()


@pytest.fixture(scope="module")
def recomputed():
    return out.compute_golden()


def test_batch_holds_every_status_at_every_lane_class(batch, recomputed):
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    for L in (2, 3, 7, 8, 9, 63, 64, 65, 129, 300):
        assert L in lengths, L
    seen = {(tri.lane_class(cs["length"]), cs["status"]) for cs in recomputed["cases"]}
    for G in (4, 16, 64):
        for status in (0, 2, 3, 4):
            assert (G, status) in seen, (G, status)
    # the unestimated cameras and the turned one are the triangulation batch's
    assert not batch["estimated"][list(tri.UNESTIMATED)].any() and batch["estimated"].sum() == batch["n_cams"] - 2
    kinds = set(batch["kind"])
    assert {"random", "mirrored", "shifted", "narrow"} <= kinds
    assert all(cs["status"] == 2 for cs in recomputed["cases"] if cs["kind"] == "mirrored")
    assert all(cs["status"] == 4 for cs in recomputed["cases"] if cs["kind"] == "narrow")


def test_hand_placed_cases_have_the_listed_statuses(batch, recomputed):
    hand = {name: recomputed["cases"][out.hand_index(batch, name)] for name in out.HAND_PLACED}
    assert [hand[k]["status"] for k in out.HAND_PLACED] == list(out.HAND_STATUS) == [1, 4, 4, 4, 0, 2, 0, 3, 4]
    assert [hand[k]["n_views"] for k in out.HAND_PLACED] == [0, 0, 1, 2, 2, 2, 3, 3, 2]
    c = out.cos_min_angle()
    under, over = hand["pair_just_under_the_angle"]["min_cos"], hand["pair_just_over_the_angle"]["min_cos"]
    assert abs(math.degrees(math.acos(under)) - (4.0 - 1e-4)) < 1e-7 and abs(math.degrees(math.acos(over)) - (4.0 + 1e-4)) < 1e-7
    assert under > c > over
    assert abs(hand["mean_just_under_16"]["mean_sq_err"] / 16.0 - (1.0 - 1e-6)) < 1e-9
    assert abs(hand["mean_just_over_16"]["mean_sq_err"] / 16.0 - (1.0 + 1e-6)) < 1e-9
    # a point exactly at a camera centre: a NaN mean that step 3 does not remove, and no pair of rays that compares
    assert hand["point_at_a_camera_centre"]["mean_sq_err"] == "nan" and hand["point_at_a_camera_centre"]["min_cos"] is None
    assert hand["all_views_unestimated"]["mean_sq_err"] == "nan"
    assert hand["not_estimated_on_input"]["mean_sq_err"] == 0.0 and not batch["point_estimated"][out.hand_index(batch, "not_estimated_on_input")]


def test_numpy_restatement_takes_the_mpmath_status_away_from_the_thresholds(recomputed):
    """in every summation order, on every case that near_threshold's rule (relative 1e-9) does not set aside -- and it sets none aside"""
    assert recomputed["num_near_threshold"] == 0            # a condition on the seed: the device test's cap of 2 hides nothing
    for t, cs in enumerate(recomputed["cases"]):
        if not cs["near_threshold"]:
            assert all(s == cs["status"] for s in cs["fp64_status"]), (t, cs["status"], cs["fp64_status"])
    print("mean spread_max %.3e over %d tracks" % (recomputed["spread_max"], len(recomputed["cases"])))
    assert 0 < recomputed["spread_max"] < 1e-9


def test_golden_file_matches_a_recomputation(recomputed):
    with open(GOLDEN) as f:
        got = json.load(f)
    for k in ("batch_seed", "orders", "mp_dps", "min_angle_degrees", "max_error_pixels", "num_near_threshold"):
        assert got[k] == recomputed[k], k
    assert got["num_near_threshold"] == 0 and len(got["cases"]) == len(recomputed["cases"])
    for a, b in zip(got["cases"], recomputed["cases"]):
        for k in ("kind", "length", "status", "n_views", "near_threshold", "fp64_status"):
            assert a[k] == b[k], (k, a, b)
        for k in ("mean_sq_err", "min_cos"):
            if isinstance(b[k], float):
                assert abs(a[k] - b[k]) <= 4 * 2.0 ** -53 * max(1.0, abs(b[k])), (k, a, b)     # the same 50-digit value, rounded
            else:
                assert a[k] == b[k], (k, a, b)
    assert got["spread_max"] == max(cs["spread"] for cs in got["cases"])
    assert 0.25 * recomputed["spread_max"] <= got["spread_max"] <= 4.0 * recomputed["spread_max"]   # rounding errors: another libm reorders them


def test_restatements_agree_on_the_order_argument(batch):
    t = batch["kind"].index("narrow")
    oc, xy = out.track_slices(batch)[t]
    a = out.outlier_fp64(batch, oc, xy, batch["points"][t], out.cos_min_angle(), 25.0)
    b = out.outlier_fp64(batch, oc, xy, batch["points"][t], out.cos_min_angle(), 25.0, order=np.arange(a.n_views)[::-1])
    assert a.status == b.status == 4 and a.n_views == b.n_views and abs(a.mean_sq_err - b.mean_sq_err) < 1e-12 and a.min_cos == b.min_cos


# ---- the C entry point on a machine without a device ----
def _call_args(b):
    dp, u32, i32, u64, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    T = len(b["track_ptr"]) - 1
    o = {"status": np.full(T, -7, dtype=np.int32), "n_views": np.full(T, -7, dtype=np.int32), "mean": np.full(T, -7.0),
         "counts": np.zeros(5, dtype=np.uint64), "ms": C.c_double(-1.0)}
    args = [b["n_cams"], b["rot_aa"].ctypes.data_as(dp), b["cam_pos"].ctypes.data_as(dp), b["intrinsics"].ctypes.data_as(dp), None, T,
            b["track_ptr"].ctypes.data_as(u64), b["obs_cam"].ctypes.data_as(u32), b["obs_xy"].ctypes.data_as(dp), b["points"].ctypes.data_as(dp),
            b["point_estimated"].ctypes.data_as(u8), 5.0, 4.0, o["status"].ctypes.data_as(i32), o["n_views"].ctypes.data_as(i32),
            o["mean"].ctypes.data_as(dp), o["counts"].ctypes.data_as(u64), C.byref(o["ms"])]
    return args, o


def test_symbol_is_exported_and_declared():
    lib = _abi.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsfm_tracks.h")).read(), flags=re.S)
    m = re.search(r"gsfm_status\s+gsfm_tracks_outlier_tracks\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    assert hasattr(lib, "gsfm_tracks_outlier_tracks")
    assert len(lib.gsfm_tracks_outlier_tracks.argtypes) == len([x for x in m.group(1).split(",") if x.strip()]) == 18
    assert callable(solver.outlier_tracks)


def test_invalid_arguments_are_rejected_before_any_device_call(batch):
    lib = _abi.load_library()
    good, _ = _call_args(batch)
    for k in (1, 2, 3, 6, 7, 8, 9, 13):                  # NULL required pointers: cameras, CSR, points, status_out
        args = list(good)
        args[k] = None
        assert lib.gsfm_tracks_outlier_tracks(*args) == _abi.ERR_INVALID_ARG, k
    ptr = batch["track_ptr"].copy()
    ptr[5], ptr[6] = ptr[6], ptr[5]
    assert ptr[6] < ptr[5]
    args = list(good)
    args[6] = ptr.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.gsfm_tracks_outlier_tracks(*args) == _abi.ERR_INVALID_ARG
    assert b"track_ptr decreases" in lib.gsfm_last_error()
    ptr1 = batch["track_ptr"] + np.uint64(1)
    args[6] = ptr1.ctypes.data_as(C.POINTER(C.c_uint64))
    args[5] = len(ptr1) - 2
    assert lib.gsfm_tracks_outlier_tracks(*args) == _abi.ERR_INVALID_ARG      # track_ptr[0] != 0
    cam = batch["obs_cam"].copy()
    cam[17] = batch["n_cams"]
    args = list(good)
    args[7] = cam.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.gsfm_tracks_outlier_tracks(*args) == _abi.ERR_INVALID_ARG
    assert b"out-of-range camera" in lib.gsfm_last_error()
    for k in (11, 12):                                    # the bound and the angle
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            args = list(good)
            args[k] = bad
            assert lib.gsfm_tracks_outlier_tracks(*args) == _abi.ERR_INVALID_ARG, (k, bad)
    with pytest.raises(solver.SolverError, match="out-of-range camera"):
        solver.outlier_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], cam, batch["obs_xy"], batch["points"])
    with pytest.raises(ValueError, match="one row per track"):
        solver.outlier_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], batch["obs_cam"], batch["obs_xy"],
                              batch["points"][:-1])


def test_calls_that_need_no_device_succeed_anywhere(batch):
    """no tracks, and no estimated track: GSFM_OK with kernel_ms = 0, status 1 and zero outputs; a call with work returns NO_DEVICE where
    there is none (on a machine with a device the same call succeeds; the device tests look at what it returns)"""
    lib = _abi.load_library()
    good, o = _call_args(batch)
    args = list(good)
    args[5] = 0
    assert lib.gsfm_tracks_outlier_tracks(*args) == 0 and o["ms"].value == 0.0 and not o["counts"].any()
    none = np.zeros(len(batch["track_ptr"]) - 1, dtype=np.uint8)
    args = list(good)
    args[10] = none.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.gsfm_tracks_outlier_tracks(*args) == 0 and o["ms"].value == 0.0
    assert (o["status"] == 1).all() and not o["n_views"].any() and not o["mean"].any()
    assert list(o["counts"]) == [0, len(none), 0, 0, 0]
    good, o = _call_args(batch)
    st = lib.gsfm_tracks_outlier_tracks(*good)
    if st == 0:                                           # this machine has a device
        assert set(o["status"]) <= {0, 1, 2, 3, 4} and int(o["counts"].sum()) == len(none)
        return
    assert st == _abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gsfm_last_error()
    assert (o["status"] == -7).all()
