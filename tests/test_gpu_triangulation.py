"""The track triangulation on the device (gsfm_tracks_triangulate, include/gsfm_tracks.h) against the 50-digit restatement
(tests/triangulation_reference.py).  The mpmath results of the parity batch and the arithmetic yardstick spread_max are read from
tests/golden/triangulation_spread.json, which tests/test_triangulation_reference.py recomputes and checks.

Status 3 (a failed Cholesky) is kept for completeness: with finite input the angle test rejects every degenerate track first, and no test
here reaches it."""
import json
import os

import numpy as np
import pytest

from globalsfmpy_amd import solver

import triangulation_reference as tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "triangulation_spread.json")
OUTPUTS = ("points", "status", "n_views", "mean_sq_err")


def triangulate(b, **over):
    a = dict(b, **over)
    return solver.triangulate_tracks(a["rot_aa"], a["cam_pos"], a["intrinsics"], a["track_ptr"], a["obs_cam"], a["obs_xy"], cam_estimated=a["estimated"],
                                     min_triangulation_angle_degrees=tri.MIN_ANGLE_DEG, max_reprojection_error_pixels=tri.MAX_ERR_PX)


def same_bytes(a, b, rows=None):
    for k in OUTPUTS:
        x, y = a[k], (b[k] if rows is None else b[k][rows])
        if not np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)):
            return False
    return True


@pytest.fixture(scope="module")
def batch():
    return tri.make_batch()


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def device(batch):
    return triangulate(batch)


def test_statuses_equal_the_high_precision_reference(batch, gold, device):
    assert gold["batch_seed"] == tri.BATCH_SEED and len(gold["cases"]) == len(batch["track_ptr"]) - 1
    left_out = [t for t, g in enumerate(gold["cases"]) if g["near_threshold"]]
    print("tracks left out (decisive quantity within 1e-9 of its threshold): %d" % len(left_out))
    assert len(left_out) <= 2 and len(left_out) == gold["num_near_threshold"] == 0
    wrong = [(t, g["length"], int(device["status"][t]), g["status"]) for t, g in enumerate(gold["cases"])
             if t not in left_out and device["status"][t] != g["status"]]
    print("status histogram on the device: %s" % dict(zip(*np.unique(device["status"], return_counts=True))))
    assert not wrong, wrong
    assert [int(device["n_views"][t]) for t in range(len(gold["cases"]))] == [g["n_views"] for g in gold["cases"]]
    hand = dict(zip(tri.HAND_PLACED, device["status"][batch["n_random"]:]))
    assert [int(hand[k]) for k in tri.HAND_PLACED] == [1, 1, 2, 0, 4, 5, 0]
    assert device["kernel_ms"] > 0


def test_points_within_four_times_the_fp64_spread(batch, gold, device):
    bound = 4.0 * gold["spread_max"]      # the lane-strided order and the butterfly are summation orders the 8 sequential ones do not sample
    worst, worst_t, n = 0.0, -1, 0
    for t, ((oc, xy), g) in enumerate(zip(tri.track_slices(batch), gold["cases"])):
        if g["status"] not in (0, 4, 5) or device["status"][t] != g["status"]:
            assert g["status"] in (0, 4, 5) or not device["points"][t].any(), t       # no point: zeros
            continue
        ref = np.array([float.fromhex(x) for x in g["point"]])
        dev = tri.relative_deviation(device["points"][t], ref, tri.origin_centroid(batch, oc))
        n += 1
        if dev > worst:
            worst, worst_t = dev, t
        tol_err = 1e-9 * max(1.0, g["mean_sq_err"])
        assert abs(device["mean_sq_err"][t] - g["mean_sq_err"]) <= tol_err, (t, device["mean_sq_err"][t], g["mean_sq_err"])
    print("points: %d compared, worst relative deviation %.3e at track %d (length %d); bound %.3e = 4 x spread_max %.3e"
          % (n, worst, worst_t, gold["cases"][worst_t]["length"], bound, gold["spread_max"]))
    assert n >= 350
    assert worst <= bound, (worst_t, worst, bound)


def permuted(b, perm):
    ptr = b["track_ptr"].astype(np.int64)
    counts = np.diff(ptr)
    rows = np.concatenate([np.arange(ptr[t], ptr[t + 1], dtype=np.int64) for t in perm]) if len(perm) else np.zeros(0, dtype=np.int64)
    new_ptr = np.concatenate([[0], np.cumsum(counts[perm])]).astype(np.uint64)
    return dict(b, track_ptr=new_ptr, obs_cam=b["obs_cam"][rows], obs_xy=b["obs_xy"][rows])


def test_two_calls_and_a_permutation_return_the_same_bytes(batch, device):
    assert same_bytes(triangulate(batch), device)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(batch["track_ptr"]) - 1)
    assert same_bytes(triangulate(permuted(batch, perm)), device, rows=perm)


def test_cam_estimated_null_equals_all_ones_and_dropping_a_camera_is_local(batch):
    ones = np.ones(batch["n_cams"], dtype=np.uint8)
    a, b = triangulate(batch, estimated=None), triangulate(batch, estimated=ones)
    assert same_bytes(a, b) and np.array_equal(a["counts"], b["counts"])
    drop = 7
    est = ones.copy()
    est[drop] = 0
    c = triangulate(batch, estimated=est)
    ptr = batch["track_ptr"].astype(np.int64)
    sees = np.array([drop in batch["obs_cam"][ptr[t]:ptr[t + 1]] for t in range(len(ptr) - 1)])
    assert 20 < sees.sum() < len(sees) - 20
    assert same_bytes({k: c[k][~sees] for k in OUTPUTS}, {k: b[k][~sees] for k in OUTPUTS})
    assert np.all(c["n_views"][sees] < b["n_views"][sees])


def test_counts_sum_to_the_tracks_and_match_the_statuses(batch, device):
    assert int(device["counts"].sum()) == len(batch["track_ptr"]) - 1
    assert list(device["counts"]) == [int(np.sum(device["status"] == k)) for k in range(6)]


def test_empty_input(batch):
    none = triangulate(batch, track_ptr=np.zeros(1, dtype=np.uint64), obs_cam=np.zeros(0, dtype=np.uint32), obs_xy=np.zeros((0, 2)))
    assert none["points"].shape == (0, 3) and none["status"].shape == (0,) and not none["counts"].any() and none["kernel_ms"] == 0.0
    # tracks of zero observations (track_ptr repeated) beside real ones
    two = permuted(batch, np.array([3, 60]))
    ptr = np.array([0, 0, two["track_ptr"][1], two["track_ptr"][1], two["track_ptr"][2], two["track_ptr"][2]], dtype=np.uint64)
    r = triangulate(two, track_ptr=ptr)
    ref = triangulate(two)
    assert list(r["status"][[0, 2, 4]]) == [1, 1, 1] and not r["points"][[0, 2, 4]].any() and not r["n_views"][[0, 2, 4]].any()
    assert same_bytes({k: r[k][[1, 3]] for k in OUTPUTS}, ref)
    only_empty = triangulate(batch, track_ptr=np.zeros(4, dtype=np.uint64), obs_cam=np.zeros(0, dtype=np.uint32), obs_xy=np.zeros((0, 2)))
    assert list(only_empty["status"]) == [1, 1, 1] and list(only_empty["counts"]) == [0, 3, 0, 0, 0, 0]
