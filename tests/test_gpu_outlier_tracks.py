"""The outlier rule on the device (gsfm_tracks_outlier_tracks, include/gsfm_tracks.h) against the 50-digit restatement
(tests/outlier_reference.py).  The mpmath results of the parity batch are read from tests/golden/outlier_tracks.json, which
tests/test_outlier_reference.py recomputes and checks.  Also here: gsfm_tracks_triangulate and gsfm_tracks_triangulate_refine still return, byte for
byte, what the commit before the angle sweep was factored out of tri_front returned on an MI355X (tests/golden/triangulation_parent_bytes.npz),
and gsfm_tracks_outlier_tracks what the commit before csrc/track_scene.hpp returned there (tests/golden/outlier_parent_bytes.npz)."""
import json
import math
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi, solver

import outlier_reference as out
import triangulation_reference as tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "outlier_tracks.json")
PARENT_BYTES = os.path.join(ROOT, "tests", "golden", "triangulation_parent_bytes.npz")
OUTLIER_PARENT_BYTES = os.path.join(ROOT, "tests", "golden", "outlier_parent_bytes.npz")
OUTPUTS = ("status", "n_views", "mean_sq_err")


def run(b, **over):
    a = dict(b, **over)
    return solver.outlier_tracks(a["rot_aa"], a["cam_pos"], a["intrinsics"], a["track_ptr"], a["obs_cam"], a["obs_xy"], a["points"],
                                 cam_estimated=a["estimated"], point_estimated=a["point_estimated"],
                                 max_reprojection_error_pixels=a.get("max_err", out.MAX_ERR_PX), min_triangulation_angle_degrees=out.MIN_ANGLE_DEG)


def raw(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bytes(a, b, rows=None):
    return all(np.array_equal(raw(a[k]), raw(b[k] if rows is None else b[k][rows])) for k in OUTPUTS)


@pytest.fixture(scope="module")
def batch():
    return out.make_batch()


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def device(batch):
    return run(batch)


@pytest.fixture(scope="module")
def device_bound_4(batch):
    """the call the two hand-placed means of 16 (1 +- 1e-6) are read from: the bound is 4 pixels"""
    return run(batch, max_err=out.MEAN16_BOUND_PX)


def merged(batch, device, device_bound_4):
    """per track the outputs of the call that ran with the track's own bound"""
    other = batch["bound_px"] != out.MAX_ERR_PX
    return {k: np.where(other, device_bound_4[k], device[k]) for k in OUTPUTS}


def test_statuses_and_view_counts_equal_the_high_precision_reference(batch, gold, device, device_bound_4):
    dev = merged(batch, device, device_bound_4)
    assert gold["batch_seed"] == out.BATCH_SEED and len(gold["cases"]) == len(batch["track_ptr"]) - 1
    left_out = [t for t, g in enumerate(gold["cases"]) if g["near_threshold"]]
    print("tracks left out (decisive quantity within 1e-9 of its threshold): %d" % len(left_out))
    assert len(left_out) <= 2 and len(left_out) == gold["num_near_threshold"] == 0
    wrong = [(t, g["kind"], g["length"], int(dev["status"][t]), g["status"]) for t, g in enumerate(gold["cases"])
             if t not in left_out and dev["status"][t] != g["status"]]
    print("status histogram on the device: %s" % dict(zip(*np.unique(dev["status"], return_counts=True))))
    assert not wrong, wrong
    assert [int(x) for x in dev["n_views"]] == [g["n_views"] for g in gold["cases"]]
    assert [int(dev["status"][out.hand_index(batch, k)]) for k in out.HAND_PLACED] == list(out.HAND_STATUS)
    assert device["kernel_ms"] > 0


def test_means_within_1e9_of_the_high_precision_reference(batch, gold, device, device_bound_4):
    dev = merged(batch, device, device_bound_4)
    worst, n_nan = 0.0, 0
    for t, g in enumerate(gold["cases"]):
        got, want = float(dev["mean_sq_err"][t]), g["mean_sq_err"]
        if want == "nan":
            assert math.isnan(got), (t, got)
            n_nan += 1
        elif isinstance(want, str):
            assert got == float(want), (t, got, want)
        else:
            tol = 1e-9 * max(1.0, want)            # the tolerance test_gpu_triangulation.py uses for this quantity
            worst = max(worst, abs(got - want) / max(1.0, want))
            assert abs(got - want) <= tol, (t, g["kind"], got, want)
    print("mean_sq_err: worst deviation %.3e of max(1, value) over %d tracks, %d NaN" % (worst, len(gold["cases"]), n_nan))
    assert n_nan == 2                              # no estimated view, and the point at a camera centre
    assert math.isnan(device["mean_sq_err"][out.hand_index(batch, "point_at_a_camera_centre")])
    t = out.hand_index(batch, "not_estimated_on_input")
    assert device["status"][t] == 1 and device["n_views"][t] == 0 and raw(device["mean_sq_err"][t:t + 1]).max() == 0


def test_the_triangulation_s_own_points_give_its_mean_byte_for_byte():
    b = tri.make_batch()
    t3 = solver.triangulate_tracks(b["rot_aa"], b["cam_pos"], b["intrinsics"], b["track_ptr"], b["obs_cam"], b["obs_xy"], cam_estimated=b["estimated"],
                                   min_triangulation_angle_degrees=tri.MIN_ANGLE_DEG, max_reprojection_error_pixels=tri.MAX_ERR_PX)
    accepted = t3["status"] == 0
    assert accepted.sum() >= 300
    r = solver.outlier_tracks(b["rot_aa"], b["cam_pos"], b["intrinsics"], b["track_ptr"], b["obs_cam"], b["obs_xy"], t3["points"],
                              cam_estimated=b["estimated"], point_estimated=accepted, max_reprojection_error_pixels=tri.MAX_ERR_PX,
                              min_triangulation_angle_degrees=tri.MIN_ANGLE_DEG)
    assert np.array_equal(raw(r["mean_sq_err"][accepted]), raw(t3["mean_sq_err"][accepted]))
    assert np.array_equal(r["n_views"][accepted], t3["n_views"][accepted])
    assert (r["status"][~accepted] == 1).all() and not r["mean_sq_err"][~accepted].any() and not r["n_views"][~accepted].any()
    # with the triangulation's own bound nothing it accepted is a bad reprojection; the angle is now taken at the point
    assert set(r["status"][accepted]) <= {0, 4} and (r["status"][accepted] == 0).sum() >= 300


def permuted(b, perm):
    ptr = b["track_ptr"].astype(np.int64)
    lengths = np.diff(ptr)[perm]
    idx = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in perm]) if len(perm) else np.zeros(0, dtype=np.int64)
    return dict(b, track_ptr=np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64), obs_cam=b["obs_cam"][idx], obs_xy=b["obs_xy"][idx],
                points=b["points"][perm], point_estimated=b["point_estimated"][perm])


def test_two_calls_and_a_permutation_return_the_same_bytes(batch, device):
    assert same_bytes(run(batch), device)
    T = len(batch["track_ptr"]) - 1
    perm = np.random.Generator(np.random.PCG64(77)).permutation(T)
    assert same_bytes(run(permuted(batch, perm)), device, rows=perm)


def test_no_camera_flags_equal_all_ones(batch):
    ones = np.ones(batch["n_cams"], dtype=np.uint8)
    a, b = run(batch, estimated=None), run(batch, estimated=ones)
    assert same_bytes(a, b) and np.array_equal(a["counts"], b["counts"])
    assert int((a["n_views"] == np.diff(batch["track_ptr"].astype(np.int64))).sum()) == len(a["n_views"]) - 1     # all but the unestimated track


def test_another_track_s_flag_changes_nothing(batch, device):
    T = len(batch["track_ptr"]) - 1
    flip = np.zeros(T, dtype=bool)
    flip[np.random.Generator(np.random.PCG64(78)).permutation(T)[:T // 2]] = True
    flags = batch["point_estimated"].copy()
    flags[flip] = 0
    r = run(batch, point_estimated=flags)
    keep = ~flip
    assert same_bytes({k: r[k][keep] for k in OUTPUTS}, device, rows=keep)
    assert (r["status"][flip] == 1).all() and raw(r["n_views"][flip]).max() == 0 and raw(r["mean_sq_err"][flip]).max() == 0


def test_counts_match_statuses(batch, device):
    T = len(batch["track_ptr"]) - 1
    assert [int(c) for c in device["counts"]] == [int((device["status"] == k).sum()) for k in range(5)]
    assert int(device["counts"].sum()) == T and all(device["counts"][k] > 0 for k in range(5))


def test_empty_zero_length_and_unestimated_input(batch, device):
    empty = dict(batch, track_ptr=np.zeros(1, dtype=np.uint64), obs_cam=np.zeros(0, dtype=np.uint32), obs_xy=np.zeros((0, 2)),
                 points=np.zeros((0, 3)), point_estimated=np.zeros(0, dtype=np.uint8))
    r = run(empty)
    assert r["kernel_ms"] == 0 and len(r["status"]) == 0 and not r["counts"].any()
    T = len(batch["track_ptr"]) - 1
    r = run(batch, point_estimated=np.zeros(T, dtype=np.uint8))
    assert r["kernel_ms"] == 0 and (r["status"] == 1).all() and not r["n_views"].any() and not r["mean_sq_err"].any() and r["counts"][1] == T
    # zero-length tracks beside real ones: status 4 with no view (Theia's empty loop), and the real ones keep their bytes; zero-length
    # tracks that are not estimated cost no launch
    ptr = batch["track_ptr"]
    with_empty = dict(batch, track_ptr=np.concatenate([[0, 0], ptr, [ptr[-1]]]).astype(np.uint64),
                      points=np.vstack([np.ones((2, 3)), batch["points"], np.ones((1, 3))]),
                      point_estimated=np.concatenate([[1, 1], batch["point_estimated"], [1]]).astype(np.uint8))
    r = run(with_empty)
    assert same_bytes({k: r[k][2:-1] for k in OUTPUTS}, device)
    for t in (0, 1, T + 2):
        assert r["status"][t] == 4 and r["n_views"][t] == 0 and math.isnan(r["mean_sq_err"][t])
    only_empty = dict(with_empty, point_estimated=np.concatenate([[0, 0], np.zeros(T, dtype=np.uint8), [0]]).astype(np.uint8))
    assert run(only_empty)["kernel_ms"] == 0


def test_triangulation_entries_return_the_parent_commit_s_bytes():
    """recorded on an MI355X from a library built before tri_angle was factored out of tri_front"""
    want = np.load(PARENT_BYTES)
    b = tri.make_batch()
    args = (b["rot_aa"], b["cam_pos"], b["intrinsics"], b["track_ptr"], b["obs_cam"], b["obs_xy"])
    kw = dict(cam_estimated=b["estimated"], min_triangulation_angle_degrees=tri.MIN_ANGLE_DEG, max_reprojection_error_pixels=tri.MAX_ERR_PX)
    got = solver.triangulate_tracks(*args, **kw)
    for k in ("points", "status", "n_views", "mean_sq_err", "counts"):
        assert got[k].dtype == want["tri_" + k].dtype and np.array_equal(raw(got[k]), raw(want["tri_" + k])), k
    got = solver.triangulate_tracks(*args, refine=True, loss=[(_abi.LOSS_HUBER, 10.0, 0.0, 0.0)], **kw)
    for k in ("points", "status", "n_views", "mean_sq_err", "counts", "iterations", "initial_cost", "final_cost", "termination"):
        assert got[k].dtype == want["refine_" + k].dtype and np.array_equal(raw(got[k]), raw(want["refine_" + k])), k
    assert int(want["tri_counts"][0]) >= 300 and int(want["refine_counts"][0]) >= 300


def half_flagged(batch):
    """the flags of test_another_track_s_flag_changes_nothing"""
    T = len(batch["track_ptr"]) - 1
    flags = batch["point_estimated"].copy()
    flags[np.random.Generator(np.random.PCG64(78)).permutation(T)[:T // 2]] = 0
    return flags


def parent_bytes_cases(batch):
    """(name, scene): the batch, the batch half flagged, and the batch's tracks of one lane class alone (two classes stay empty)"""
    lanes = np.array([tri.lane_class(int(n)) for n in np.diff(batch["track_ptr"].astype(np.int64))])
    yield "all", batch
    yield "half", dict(batch, point_estimated=half_flagged(batch))
    for g in (4, 16, 64):
        yield "lanes%d" % g, permuted(batch, np.flatnonzero(lanes == g))


def test_outlier_rule_returns_the_parent_commit_s_bytes(batch):
    """recorded on an MI355X from a library built before the scene slab, the checks and the lane-class launcher moved to csrc/track_scene.hpp
    (tools/make_track_scene_golden.py)"""
    want = np.load(OUTLIER_PARENT_BYTES)
    sizes = {}
    for name, scene in parent_bytes_cases(batch):
        got = run(scene)
        sizes[name] = len(got["status"])
        for k in OUTPUTS + ("counts",):
            assert got[k].dtype == want[name + "_" + k].dtype and np.array_equal(raw(got[k]), raw(want[name + "_" + k])), (name, k)
    T = sizes["all"]
    assert min(sizes.values()) >= 20 and sizes["lanes4"] + sizes["lanes16"] + sizes["lanes64"] == T
    assert int(want["half_counts"][1]) >= T // 2 and int(want["all_counts"][1]) == 1
