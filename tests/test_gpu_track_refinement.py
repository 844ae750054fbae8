"""The track triangulation with the per-track refinement on the device (gsfm_tracks_triangulate_refine, include/gsfm_tracks.h) against the
50-digit restatement (tests/track_refinement_reference.py).  The mpmath results of the parity batch and the arithmetic yardstick spread_max
are read from tests/golden/track_refinement_spread.json, which tests/test_track_refinement_reference.py recomputes and checks.

The bound of test_points_and_costs_within_four_times_the_fp64_spread is 4 x spread_max = 3.0e-10; the test prints the device's worst
deviations, which the JSON's "device_measured" and DESIGN.md section 15 record.

Tukey 10, Geman-McClure (10, 0.5) and SoftLOne 10 run on a sub-batch of 62 tracks (track_refinement_reference.make_sub_batch: the hand-placed
tracks, per lane class the slowest and the fastest under Huber, and four tracks placed for Tukey's cut) against
tests/golden/track_refinement_losses.json, each loss within 4 x its own spread_max."""
import json
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi, solver

import track_refinement_reference as ref
import triangulation_reference as tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "track_refinement_spread.json")
BASE = ("points", "status", "n_views", "mean_sq_err")
OUTPUTS = BASE + ("iterations", "initial_cost", "final_cost", "termination")
HUBER10, TRIVIAL = [(_abi.LOSS_HUBER, 10.0)], [(_abi.LOSS_TRIVIAL,)]
GOLDEN_LOSSES = os.path.join(ROOT, "tests", "golden", "track_refinement_losses.json")
SUB_NODES = {"tukey": [(_abi.LOSS_TUKEY, 10.0)], "geman": [(_abi.LOSS_GEMAN_MCCLURE, 10.0, 0.5)], "softl1": [(_abi.LOSS_SOFT_L1, 10.0)]}


def run(b, refine=True, loss=HUBER10, max_num_iterations=100, options=None, **over):
    a = dict(b, **over)
    return solver.triangulate_tracks(a["rot_aa"], a["cam_pos"], a["intrinsics"], a["track_ptr"], a["obs_cam"], a["obs_xy"], cam_estimated=a["estimated"],
                                     min_triangulation_angle_degrees=tri.MIN_ANGLE_DEG, max_reprojection_error_pixels=tri.MAX_ERR_PX,
                                     refine=refine, loss=loss, max_num_iterations=max_num_iterations, **(options or {}))


def permuted(b, perm):
    ptr = b["track_ptr"].astype(np.int64)
    counts = np.diff(ptr)
    rows = np.concatenate([np.arange(ptr[t], ptr[t + 1], dtype=np.int64) for t in perm])
    new_ptr = np.concatenate([[0], np.cumsum(counts[perm])]).astype(np.uint64)
    return dict(b, track_ptr=new_ptr, obs_cam=b["obs_cam"][rows], obs_xy=b["obs_xy"][rows])


def same_bytes(a, b, rows=None, keys=OUTPUTS):
    for k in keys:
        x, y = a[k], (b[k] if rows is None else b[k][rows])
        if not np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)):
            return False
    return True


@pytest.fixture(scope="module")
def batch():
    return ref.make_batch()


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def device(batch):
    return run(batch)


@pytest.fixture(scope="module")
def unrefined(batch):
    return run(batch, refine=False)


def test_decisions_equal_the_high_precision_reference(batch, gold, device):
    cases = gold["cases"]
    assert gold["hand_seed"] == ref.HAND_SEED and len(cases) == len(batch["track_ptr"]) - 1
    flagged = [t for t, g in enumerate(cases) if g["near"]]
    print("tracks left out (a decision within 1e-9 of its threshold): %d" % len(flagged))
    assert len(flagged) == gold["num_near"] and len(flagged) <= ref.MAX_FLAGGED_FRACTION * len(cases)
    wrong = [(t, g["length"], (int(device["status"][t]), int(device["termination"][t]), int(device["iterations"][t])), (g["status"], g["termination"], g["iterations"]))
             for t, g in enumerate(cases)
             if t not in flagged and (device["status"][t], device["termination"][t], device["iterations"][t]) != (g["status"], g["termination"], g["iterations"])]
    print("status histogram on the device: %s; iterations mean %.2f max %d" % (dict(zip(*np.unique(device["status"], return_counts=True))),
                                                                              device["iterations"][device["termination"] >= 0].mean(), device["iterations"].max()))
    assert not wrong, wrong
    assert [int(x) for x in device["n_views"]] == [g["n_views"] for g in cases]
    assert list(device["counts"]) == [int(np.sum(device["status"] == k)) for k in range(7)] and device["kernel_ms"] > 0


def test_points_and_costs_within_four_times_the_fp64_spread(batch, gold, device):
    bound = 4.0 * gold["spread_max"]      # the lane-strided order and the butterfly are summation orders the 8 sequential ones do not sample
    worst, worst_t, worst_c, worst_ct, n = 0.0, -1, 0.0, -1, 0
    for t, ((oc, xy), g) in enumerate(zip(tri.track_slices(batch), gold["cases"])):
        if g["near"] or g["status"] not in (0, 4, 5) or device["status"][t] != g["status"]:
            assert g["status"] in (0, 4, 5) or not device["points"][t].any(), t       # no point: zeros
            continue
        point = np.array([float.fromhex(x) for x in g["point"]])
        dev = tri.relative_deviation(device["points"][t], point, tri.origin_centroid(batch, oc))
        n += 1
        if dev > worst:
            worst, worst_t = dev, t
        if g["final_cost"] > 1e-12:            # below: the cost is the rounding of the pixels (the golden file's rule)
            dc = ref.relative_cost_deviation(device["final_cost"][t], g["final_cost"])
            if dc > worst_c:
                worst_c, worst_ct = dc, t
        assert device["final_cost"][t] <= device["initial_cost"][t], t
    print("points: %d compared, worst relative deviation %.3e at track %d (length %d); final costs: worst %.3e at track %d (length %d); bound %.3e = 4 x spread_max %.3e"
          % (n, worst, worst_t, gold["cases"][worst_t]["length"], worst_c, worst_ct, gold["cases"][worst_ct]["length"], bound, gold["spread_max"]))
    assert n >= 350
    assert worst <= bound, (worst_t, worst, bound)
    assert worst_c <= bound, (worst_ct, worst_c, bound)


def test_refine_off_returns_the_bytes_of_the_triangulation(batch, unrefined):
    old = solver.triangulate_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], batch["obs_cam"], batch["obs_xy"],
                                    cam_estimated=batch["estimated"])
    assert sorted(unrefined) == sorted(old) and same_bytes(unrefined, old, keys=BASE) and np.array_equal(unrefined["counts"], old["counts"])
    # the C entry with options.refine = 0
    import ctypes as C
    lib = _abi.load_library()
    opt = _abi.TrackRefineOptions()
    lib.gsfm_tracks_refine_default_options(C.byref(opt))
    opt.refine = 0
    T = len(batch["track_ptr"]) - 1
    pts, st, nv, err = np.zeros((T, 3)), np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros(T)
    it, term, counts = np.full(T, 7, dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros(7, dtype=np.uint64)
    dp, u32, i32, u64 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    prog, n = _abi.make_program(HUBER10)
    rc = lib.gsfm_tracks_triangulate_refine(batch["n_cams"], batch["rot_aa"].ctypes.data_as(dp), batch["cam_pos"].ctypes.data_as(dp),
                                            batch["intrinsics"].ctypes.data_as(dp), batch["estimated"].ctypes.data_as(C.POINTER(C.c_uint8)), T,
                                            batch["track_ptr"].ctypes.data_as(u64), batch["obs_cam"].ctypes.data_as(u32), batch["obs_xy"].ctypes.data_as(dp),
                                            tri.MIN_ANGLE_DEG, tri.MAX_ERR_PX, C.byref(opt), prog, n, pts.ctypes.data_as(dp), st.ctypes.data_as(i32),
                                            nv.ctypes.data_as(i32), err.ctypes.data_as(dp), it.ctypes.data_as(i32), None, None, term.ctypes.data_as(i32),
                                            counts.ctypes.data_as(u64), None)
    assert rc == 0 and same_bytes({"points": pts, "status": st, "n_views": nv, "mean_sq_err": err}, old, keys=BASE)
    assert not it.any() and np.all(term == -1) and list(counts[:6]) == list(old["counts"]) and counts[6] == 0


def test_zero_iterations_return_the_midpoint_with_its_gate(batch, unrefined):
    r = run(batch, max_num_iterations=0)
    assert same_bytes(r, unrefined, keys=BASE)
    refined = unrefined["status"] != 1
    refined &= (unrefined["status"] != 2) & (unrefined["status"] != 3)
    assert not r["iterations"].any() and np.all(r["termination"][~refined] == -1)
    assert set(r["termination"][refined]) <= {ref.GRADIENT_TOLERANCE, ref.NO_CONVERGENCE} and np.all(r["initial_cost"][refined] == r["final_cost"][refined])


def test_two_calls_and_a_permutation_return_the_same_bytes(batch, device):
    assert same_bytes(run(batch), device)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(batch["track_ptr"]) - 1)
    assert same_bytes(run(permuted(batch, perm)), device, rows=perm)


def test_a_track_alone_returns_its_bytes_of_the_batch(batch, gold, device):
    """n_tracks = 1 leaves 63, 15 or no dead groups beside the track; inside the batch it shares its wavefront with faster and slower ones"""
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    its = np.array([g["iterations"] for g in gold["cases"]])
    picks = [ref.hand_index(batch, k) for k in ref.HAND_PLACED]
    for G in (4, 16, 64):                                   # per class the slowest track
        of_class = [t for t in range(batch["n_base"]) if tri.lane_class(lengths[t]) == G]
        picks.append(max(of_class, key=lambda t: its[t]))
    assert its[picks].max() >= 40 and its[picks].min() <= 2
    for t in picks:
        alone = run(permuted(batch, np.array([t])))
        assert same_bytes(alone, device, rows=np.array([t])), (t, int(lengths[t]))


def test_sixty_five_short_tracks_fill_a_block_and_one_group(batch, device):
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    short = np.flatnonzero(lengths <= tri.LEN_G4)[:65]
    assert len(short) == 65                                 # 64 groups of 4 lanes make a block: the second block holds one live group
    assert same_bytes(run(permuted(batch, short)), device, rows=short)


def test_hand_placed_tracks(batch, device, unrefined):
    t = ref.hand_index(batch, "midpoint_fails_the_gate_refined_passes")
    assert unrefined["status"][t] == 5 and device["status"][t] == 0 and device["mean_sq_err"][t] < 0.5 * unrefined["mean_sq_err"][t]
    t = ref.hand_index(batch, "one_outlier_observation")
    triv = run(permuted(batch, np.array([t])), loss=TRIVIAL)
    assert triv["status"][0] == 0 and device["status"][t] == 0 and np.linalg.norm(triv["points"][0] - device["points"][t]) > 1e-3
    none = run(permuted(batch, np.array([t])), loss=None)                       # Ceres' NULL loss is the trivial one
    assert same_bytes(none, triv)
    t = ref.hand_index(batch, "noise_free")
    assert device["status"][t] == 0 and 0 < device["iterations"][t] <= 2
    assert device["status"][ref.hand_index(batch, "two_views")] == 0 and device["n_views"][ref.hand_index(batch, "two_views")] == 2
    t = ref.hand_index(batch, "unestimated_in_the_middle")
    assert device["status"][t] == 0 and device["n_views"][t] == 4
    for L in (8, 9, 64, 65, 130):
        t = ref.hand_index(batch, "length_%d" % L)
        assert device["status"][t] == 0 and device["termination"][t] == ref.FUNCTION_TOLERANCE, L


# ---- Tukey, Geman-McClure and SoftLOne on the sub-batch ----
@pytest.fixture(scope="module")
def gold_losses():
    with open(GOLDEN_LOSSES) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sub(batch, gold, gold_losses):
    b = ref.make_sub_batch(batch, gold["cases"])
    assert [int(t) for t in b["picks"]] == gold_losses["picks"] and gold_losses["hand_placed"] == list(ref.SUB_HAND_PLACED)
    return b


@pytest.fixture(scope="module")
def sub_device(sub):
    return {name: run(sub, loss=nodes) for name, nodes in SUB_NODES.items()}


def _point(case):
    return np.array([float.fromhex(x) for x in case["point"]])


@pytest.mark.parametrize("name", sorted(SUB_NODES))
def test_sub_batch_decisions_points_and_costs_per_loss(name, sub, gold_losses, sub_device):
    doc, dev = gold_losses["losses"][name], sub_device[name]
    cases = doc["cases"]
    assert doc["loss"] == json.loads(json.dumps(ref.SUB_LOSSES[name])) and len(cases) == len(sub["track_ptr"]) - 1
    flagged = [t for t, g in enumerate(cases) if g["near"]]
    assert len(flagged) == doc["num_near"] and len(flagged) <= max(1, int(ref.MAX_FLAGGED_FRACTION * len(cases)))     # (one track: the full batch's cap)
    wrong = [(t, g["length"], (int(dev["status"][t]), int(dev["termination"][t]), int(dev["iterations"][t])), (g["status"], g["termination"], g["iterations"]))
             for t, g in enumerate(cases)
             if t not in flagged and (dev["status"][t], dev["termination"][t], dev["iterations"][t]) != (g["status"], g["termination"], g["iterations"])]
    assert not wrong, wrong
    assert [int(x) for x in dev["n_views"]] == [g["n_views"] for g in cases]
    bound = 4.0 * doc["spread_max"]
    worst, worst_t, worst_c, worst_ct, n = 0.0, -1, 0.0, -1, 0
    for t, ((oc, xy), g) in enumerate(zip(tri.track_slices(sub), cases)):
        if g["near"] or g["status"] not in (0, 4, 5):
            assert g["status"] in (0, 4, 5) or not dev["points"][t].any(), t
            continue
        d = tri.relative_deviation(dev["points"][t], _point(g), tri.origin_centroid(sub, oc))
        n += 1
        if d > worst:
            worst, worst_t = d, t
        if g["final_cost"] > 1e-12:
            dc = ref.relative_cost_deviation(dev["final_cost"][t], g["final_cost"])
            if dc > worst_c:
                worst_c, worst_ct = dc, t
        assert dev["final_cost"][t] <= dev["initial_cost"][t], t
    print("%s: %d tracks left out, %d compared, points worst %.3e at track %d (length %d); final costs worst %.3e at track %d (length %d); bound %.3e = 4 x spread_max %.3e"
          % (name, len(flagged), n, worst, worst_t, cases[worst_t]["length"], worst_c, worst_ct, cases[worst_ct]["length"], bound, doc["spread_max"]))
    assert n >= 50
    assert worst <= bound, (worst_t, worst, bound)
    assert worst_c <= bound, (worst_ct, worst_c, bound)


def test_tukey_on_the_tracks_placed_for_its_cut(sub, gold_losses, sub_device):
    dev = sub_device["tukey"]
    # every observation beyond the cut at the midpoint: g = 0, no iteration, the midpoint's bytes
    t = ref.sub_index(sub, "all_beyond_the_tukey_cut")
    mid = run(sub, refine=False)
    assert dev["iterations"][t] == 0 and dev["termination"][t] == ref.GRADIENT_TOLERANCE and dev["final_cost"][t] == dev["initial_cost"][t] > 0
    assert dev["points"][t].tobytes() == mid["points"][t].tobytes() and dev["status"][t] == mid["status"][t]
    assert sub_device["geman"]["iterations"][t] > 0
    # one observation 30 px off, exact inliers: it weighs nothing under Tukey.  Tukey's point is far from Huber's, and with both refinements
    # run to their minimiser (SUB_CONVERGED; at the default tolerances they stop a step short of it) Tukey's point of the track WITH the
    # outlier is the trivial loss's point of the track WITHOUT it within 4 x spread_max, each also that close to its 50-digit point
    t = ref.sub_index(sub, "one_beyond_the_cut")
    oc, xy = tri.track_slices(sub)[t]
    huber = run(permuted(sub, np.array([t])), loss=HUBER10)
    assert dev["status"][t] == 0 and huber["status"][0] == 0 and np.linalg.norm(dev["points"][t] - huber["points"][0]) > 1e-3
    oc1, xy1 = ref.without_observation(oc, xy, ref.SUB_OUTLIER_PLACE)
    alone = dict(sub, track_ptr=np.array([0, len(oc1)], dtype=np.uint64), obs_cam=np.ascontiguousarray(oc1), obs_xy=np.ascontiguousarray(xy1))
    with_it = run(permuted(sub, np.array([t])), loss=SUB_NODES["tukey"], options=ref.SUB_CONVERGED)
    without = run(alone, loss=TRIVIAL, options=ref.SUB_CONVERGED)
    assert with_it["status"][0] == 0 and without["status"][0] == 0
    bound = 4.0 * gold_losses["losses"]["tukey"]["spread_max"]
    centroid = tri.origin_centroid(sub, oc)
    want = {k: np.array([float.fromhex(x) for x in v]) for k, v in gold_losses["without_the_outlier"].items()}
    devs = {"Tukey with / trivial without": tri.relative_deviation(with_it["points"][0], without["points"][0], centroid),
            "Tukey with / its 50 digits": tri.relative_deviation(with_it["points"][0], want["tukey_with_it"], centroid),
            "trivial without / its 50 digits": tri.relative_deviation(without["points"][0], want["trivial"], centroid)}
    print("one_beyond_the_cut, converged: %s; bound %.3e; iterations %d / %d" % ("  ".join("%s %.3e" % kv for kv in devs.items()), bound,
                                                                               with_it["iterations"][0], without["iterations"][0]))
    assert max(devs.values()) <= bound, devs
    assert dev["status"][ref.sub_index(sub, "at_the_cut")] == 0 and dev["status"][ref.sub_index(sub, "length_65_mixed")] == 0


def test_tukey_two_calls_a_permutation_and_tracks_alone_return_the_same_bytes(sub, sub_device):
    dev, nodes = sub_device["tukey"], SUB_NODES["tukey"]
    assert same_bytes(run(sub, loss=nodes), dev)
    perm = np.random.Generator(np.random.PCG64(6)).permutation(len(sub["track_ptr"]) - 1)
    assert same_bytes(run(permuted(sub, perm), loss=nodes), dev, rows=perm)
    picks = [ref.sub_index(sub, k) for k in ref.SUB_HAND_PLACED] + [int(np.argmax(dev["iterations"]))]
    for t in picks:
        assert same_bytes(run(permuted(sub, np.array([t])), loss=nodes), dev, rows=np.array([t])), t
