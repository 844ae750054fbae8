"""The two restatements of the track triangulation (tests/triangulation_reference.py) against each other, the yardstick of the device test
(tests/golden/triangulation_spread.json, written by tools/make_triangulation_golden.py and held here to a recomputation), the launch-order
helper, synth.make_tracks, and what gsfm_tracks_triangulate answers on a machine without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from globalsfmpy_amd import _abi, solver, synth

import triangulation_reference as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "triangulation_spread.json")


@pytest.fixture(scope="module")
def batch():
    return tri.make_batch()


@pytest.fixture(scope="module")
def recomputed(batch):
    return tri.compute_golden(batch)


def test_batch_holds_the_lengths_and_the_hand_placed_cases(batch, recomputed):
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    assert batch["n_cams"] == 40 and 380 <= len(lengths) <= 420
    for L in (2, 3, tri.LEN_G4 - 1, tri.LEN_G4, tri.LEN_G4 + 1, tri.LEN_G16 - 1, tri.LEN_G16, tri.LEN_G16 + 1, 129, 300):
        assert L in lengths[:batch["n_random"]], L
    hand = dict(zip(tri.HAND_PLACED, recomputed["cases"][batch["n_random"]:]))
    assert [hand[k]["status"] for k in tri.HAND_PLACED] == [1, 1, 2, 0, 4, 5, 0]
    assert [hand[k]["n_views"] for k in tri.HAND_PLACED] == [0, 1, 2, 2, 2, 3, 3]
    c = tri.cos_min_angle()
    assert 0 < hand["pair_just_under_the_angle"]["min_cos"] - c < 1e-6 and 0 < c - hand["pair_just_over_the_angle"]["min_cos"] < 1e-6
    # the random part skips unestimated cameras at every length, and every status but 3 occurs
    ptr = batch["track_ptr"].astype(np.int64)
    for L in (3, tri.LEN_G16, 300):
        assert any(lengths[t] == L and not batch["estimated"][batch["obs_cam"][ptr[t]:ptr[t + 1]]].all() for t in range(batch["n_random"])), L
    assert set(cs["status"] for cs in recomputed["cases"]) == {0, 1, 2, 4, 5}


def test_numpy_restatement_agrees_with_mpmath_on_the_batch(recomputed):
    """statuses in every summation order; the points through the spread, which is a few hundred ulps at the worst"""
    assert recomputed["num_near_threshold"] == 0            # a condition on the seed: the status test leaves no track out
    for t, cs in enumerate(recomputed["cases"]):
        assert all(s == cs["status"] for s in cs["fp64_status"]), (t, cs["status"], cs["fp64_status"])
    print("spread_max %.3e over %d tracks" % (recomputed["spread_max"], len(recomputed["cases"])))
    assert 0 < recomputed["spread_max"] < 1e-11


def test_golden_file_matches_a_recomputation(recomputed):
    with open(GOLDEN) as f:
        got = json.load(f)
    for k in ("batch_seed", "orders", "mp_dps", "min_angle_degrees", "max_error_pixels", "num_near_threshold"):
        assert got[k] == recomputed[k], k
    assert got["num_near_threshold"] == 0 and len(got["cases"]) == len(recomputed["cases"])
    for a, b in zip(got["cases"], recomputed["cases"]):
        for k in ("length", "status", "n_views", "near_threshold"):
            assert a[k] == b[k], (k, a, b)
        pa, pb = np.array([float.fromhex(x) for x in a["point"]]), np.array([float.fromhex(x) for x in b["point"]])
        assert np.max(np.abs(pa - pb)) <= 4 * 2.0 ** -53 * max(1.0, np.max(np.abs(pb)))      # the same 50-digit value, rounded
    assert got["spread_max"] == max(cs["spread"] for cs in got["cases"])
    assert 0.25 * recomputed["spread_max"] <= got["spread_max"] <= 4.0 * recomputed["spread_max"]   # rounding errors: another libm reorders them


def test_restatements_on_a_noise_free_track_recover_the_point():
    g = synth.make_tracks(12, 20, 3, lengths=(2, 5, 9), noise_px=0.0)
    ptr = g["track_ptr"].astype(np.int64)
    for t in range(20):
        oc, xy = g["obs_cam"][ptr[t]:ptr[t + 1]], g["obs_xy"][ptr[t]:ptr[t + 1]]
        for fn in (tri.triangulate_fp64, tri.triangulate_mp):
            r = fn(g, oc, xy, tri.cos_min_angle(0.01), 1.0)
            assert r.status == 0 and r.n_views == len(oc) and np.linalg.norm(r.point - g["gt_points"][t]) < 1e-9 and float(r.mean_sq_err) < 1e-12
    # the order argument changes the rounding, not the result
    oc, xy = g["obs_cam"][ptr[19]:ptr[20]], g["obs_xy"][ptr[19]:ptr[20]]
    a = tri.triangulate_fp64(g, oc, xy, tri.cos_min_angle(), 225.0)
    b = tri.triangulate_fp64(g, oc, xy, tri.cos_min_angle(), 225.0, order=np.arange(len(oc))[::-1])
    assert a.status == b.status and np.linalg.norm(a.point - b.point) < 1e-12


@pytest.mark.parametrize("lengths", [[], [0], [2], [8, 9, 8, 64, 65, 64, 9, 0, 1000, 65, 3], list(range(0, 140)), [5] * 7, [70, 70, 9, 9]])
def test_launch_order_of_hand_made_length_lists(lengths):
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    order, begin = solver.track_launch_order(ptr)
    want_order, want_begin = tri.launch_order(lengths)
    assert list(order) == want_order and list(begin) == want_begin
    assert sorted(order) == list(range(len(lengths)))
    for k, G in enumerate((4, 16, 64)):
        part = [lengths[t] for t in order[int(begin[k]):int(begin[k + 1])]]
        assert all(tri.lane_class(x) == G for x in part) and part == sorted(part, reverse=True)


def test_lane_class_boundaries_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "gsfm_tracks.h")).read()
    assert "len <= 8: G = 4" in hdr and "9 <= len <= 64: G = 16" in hdr and "len >= 65: G = 64" in hdr
    assert [tri.lane_class(x) for x in (0, 2, 8, 9, 64, 65, 5000)] == [4, 4, 4, 16, 16, 64, 64]
    bad = np.array([0, 3, 2], dtype=np.uint64)
    with pytest.raises(solver.SolverError, match="track_ptr decreases"):
        solver.track_launch_order(bad)


def test_make_tracks_is_reproducible():
    a = synth.make_tracks(30, 500, 11, lengths=(2, 3, 9, 70), length_weights=(0.5, 0.3, 0.15, 0.05), outlier_frac=0.05)
    b = synth.make_tracks(30, 500, 11, lengths=(2, 3, 9, 70), length_weights=(0.5, 0.3, 0.15, 0.05), outlier_frac=0.05)
    c = synth.make_tracks(30, 500, 12, lengths=(2, 3, 9, 70), length_weights=(0.5, 0.3, 0.15, 0.05), outlier_frac=0.05)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["obs_xy"], c["obs_xy"])
    lengths = np.diff(a["track_ptr"].astype(np.int64))
    assert set(lengths) == {2, 3, 9, 70} and a["obs_cam"].max() < 30 and a["obs_xy"].shape == (int(a["track_ptr"][-1]), 2)
    assert 0.02 < a["is_outlier"].mean() < 0.09
    ptr = a["track_ptr"].astype(np.int64)
    for t in np.flatnonzero(lengths <= 30)[:50]:      # up to n_cams observations a track's cameras are distinct
        assert len(set(a["obs_cam"][ptr[t]:ptr[t + 1]])) == lengths[t]
    # every point lies in front of every camera that observes it, and inlier pixels are within a few noise sigmas of the projection
    R = synth.aa_to_matrix(a["rot_aa"])
    tr = np.repeat(np.arange(500), lengths)
    p = np.einsum("eij,ej->ei", R[a["obs_cam"]], a["gt_points"][tr] - a["cam_pos"][a["obs_cam"]])
    assert p[:, 2].min() > 3.0
    proj = a["intrinsics"][a["obs_cam"], :1] * p[:, :2] / p[:, 2:] + a["intrinsics"][a["obs_cam"], 1:]
    dev = np.linalg.norm(proj - a["obs_xy"], axis=1)
    assert dev[~a["is_outlier"]].max() < 5.0 and dev[a["is_outlier"]].min() > 40.0


# ---- the C entry point on a machine without a device ----
def _call_args(b):
    dp, u32, i32, u64 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    T = len(b["track_ptr"]) - 1
    out = {"points": np.zeros((T, 3)), "status": np.zeros(T, dtype=np.int32)}
    args = [b["n_cams"], b["rot_aa"].ctypes.data_as(dp), b["cam_pos"].ctypes.data_as(dp), b["intrinsics"].ctypes.data_as(dp), None, T,
            b["track_ptr"].ctypes.data_as(u64), b["obs_cam"].ctypes.data_as(u32), b["obs_xy"].ctypes.data_as(dp), 4.0, 15.0,
            out["points"].ctypes.data_as(dp), out["status"].ctypes.data_as(i32), None, None, None, None]
    return args, out


def test_symbol_is_exported_and_declared():
    lib = _abi.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsfm_tracks.h")).read(), flags=re.S)
    for name, count in (("gsfm_tracks_triangulate", 17), ("gsfm_tracks_launch_order", 4)):
        m = re.search(r"gsfm_status\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == len([x for x in m.group(1).split(",") if x.strip()]) == count
    assert callable(solver.triangulate_tracks)


def test_invalid_arguments_are_rejected_before_any_device_call(batch):
    lib = _abi.load_library()
    good, _ = _call_args(batch)
    for k in (1, 2, 3, 6, 7, 8, 11, 12):                 # NULL required pointers
        args = list(good)
        args[k] = None
        assert lib.gsfm_tracks_triangulate(*args) == _abi.ERR_INVALID_ARG, k
    ptr = batch["track_ptr"].copy()
    ptr[5], ptr[6] = ptr[6], ptr[5]
    assert ptr[6] < ptr[5]
    args = list(good)
    args[6] = ptr.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.gsfm_tracks_triangulate(*args) == _abi.ERR_INVALID_ARG
    assert b"track_ptr decreases" in lib.gsfm_last_error()
    ptr1 = batch["track_ptr"] + np.uint64(1)
    args[6] = ptr1.ctypes.data_as(C.POINTER(C.c_uint64))
    args[5] = len(ptr1) - 2
    assert lib.gsfm_tracks_triangulate(*args) == _abi.ERR_INVALID_ARG      # track_ptr[0] != 0
    cam = batch["obs_cam"].copy()
    cam[17] = batch["n_cams"]
    args = list(good)
    args[7] = cam.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.gsfm_tracks_triangulate(*args) == _abi.ERR_INVALID_ARG
    assert b"out-of-range camera" in lib.gsfm_last_error()
    for k in (9, 10):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            args = list(good)
            args[k] = bad
            assert lib.gsfm_tracks_triangulate(*args) == _abi.ERR_INVALID_ARG, (k, bad)
    with pytest.raises(solver.SolverError, match="out-of-range camera"):
        solver.triangulate_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], cam, batch["obs_xy"])


def test_valid_call_without_a_device_returns_no_device(batch):
    """on a machine with a device the same call succeeds; the device tests look at what it returns"""
    lib = _abi.load_library()
    good, out = _call_args(batch)
    st = lib.gsfm_tracks_triangulate(*good)
    if st == 0:                                           # this machine has a device
        assert set(out["status"]) <= {0, 1, 2, 3, 4, 5} and out["points"].any()
        return
    assert st == _abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gsfm_last_error()
    assert not out["points"].any()
    # no tracks: nothing to do, with or without a device
    args = list(good)
    args[5] = 0
    assert lib.gsfm_tracks_triangulate(*args) == 0
