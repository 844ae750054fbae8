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
GOLDEN_LOSSES = os.path.join(ROOT, "tests", "golden", "track_refinement_losses.json")
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


# ---- Tukey, Geman-McClure and SoftLOne on the sub-batch ----
@pytest.fixture(scope="module")
def sub(batch, recomputed):
    return ref.make_sub_batch(batch, recomputed["cases"])


@pytest.fixture(scope="module")
def sub_recomputed(sub):
    return ref.compute_sub_golden(sub)


def _hexpoint(p):
    return np.array([float.fromhex(x) for x in p])


@pytest.mark.parametrize("ops", [ref._Fp64, ref._Mp])
def test_loss_rows_against_the_loss_classes(ops):
    """_rho on either number type against loss_functions' classes (pinned to the reference project's vectors by tests/test_oracle_golden.py) at
    s = 0, inside, at the cut, beyond.  Bound: a few roundings of float64 -- for Tukey of each function's largest value (the class forms
    v = 1 - s / a^2 and 1 - v^3 in float64, absolute errors of u that the 50-digit tier does not share), else of the value."""
    import mpmath
    from globalsfmpy_amd import loss_functions as LF
    u = 2.0 ** -53
    with mpmath.workdps(tri.MP_DPS):
        for loss, cls, floor in ((ref.TUKEY10, LF.TukeyLoss(10.0), (100.0 / 6, 0.5, 0.01)), (ref.GEMAN10, LF.GemanMcClureLoss(10.0, 0.5), (0.0, 0.0, 0.0)),
                                 (ref.SOFTL1_10, LF.SoftLOneLoss(10.0), (0.0, 0.0, 0.0)), (ref.HUBER10, LF.HuberLoss(10.0), (0.0, 0.0, 0.0))):
            for s in (0.0, 1e-3, 37.0, 99.999, 100.0, 100.0 + 1e-9, 2500.0, 1e8):
                want = [0.0, 0.0, 0.0]
                cls.Evaluate(s, want)
                got = ref._rho(loss, ops.num(s), ops)
                for k in range(3):
                    # (SoftLOne's rho = 2 b (sqrt(1 + s / b) - 1) cancels at small s in float64: an absolute 2 b u)
                    tol = 8 * u * max(abs(want[k]), floor[k], 200.0 if (loss is ref.SOFTL1_10 and k == 0) else 0.0)
                    assert abs(float(got[k]) - want[k]) <= tol, (loss, s, k, float(got[k]), want[k])
        t = ref._rho(ref.TUKEY10, ops.num(100.0 + 1e-9), ops)
        assert t[1] == 0 and t[2] == 0 and float(t[0]) == 100.0 / 6


@pytest.mark.parametrize("ops", [ref._Fp64, ref._Mp])
def test_corrected_gradient_is_the_gradient_of_the_robustified_cost(sub, ops):
    """sum J~^T r~ = sum rho' J^T r on both number types, for every loss, at the midpoint of tracks that have observations on both sides of
    the Tukey cut (J^T r and s per observation from the trivial-loss pass of a one-observation track)."""
    import mpmath
    sl = tri.track_slices(sub)
    with mpmath.workdps(tri.MP_DPS), np.errstate(all="ignore"):
        for name in ("one_beyond_the_cut", "length_65_mixed", "at_the_cut"):
            oc, xy = sl[ref.sub_index(sub, name)]
            X = [ops.num(v) for v in ref.refine_fp64(sub, oc, xy, COS, MAX_SQ, refine=False).point]
            singles = [ref._Track(sub, oc[k:k + 1], xy[k:k + 1], ops).passes(X, ref.TRIVIAL, None) for k in range(len(oc))]
            for loss in (ref.HUBER10, ref.SOFTL1_10, ref.TUKEY10, ref.GEMAN10):
                got = ref._Track(sub, oc, xy, ops).passes(X, loss, None)
                rho = [ref._rho(loss, 2 * one[9], ops) for one in singles]
                if loss is ref.TUKEY10 and name != "at_the_cut":
                    assert any(r[1] == 0 for r in rho) and any(r[1] > 0 for r in rho)
                for c in range(3):
                    want = sum(r[1] * one[6 + c] for r, one in zip(rho, singles))
                    scale = sum(abs(r[1] * one[6 + c]) for r, one in zip(rho, singles))
                    assert abs(float(got[6 + c] - want)) <= 1e-12 * float(scale), (name, loss, c)
                assert abs(float(got[9] - sum(r[0] for r in rho) / 2)) <= 1e-12 * float(got[9])


def test_sub_batch_holds_its_tracks_and_the_reference_flags_none(batch, sub, sub_recomputed):
    lengths = np.diff(sub["track_ptr"].astype(np.int64))
    assert len(lengths) == len(ref.HAND_PLACED) + 6 * ref.SUB_PER_CLASS + len(ref.SUB_HAND_PLACED) == 62
    assert sub["picks"][:len(ref.HAND_PLACED)] == [ref.hand_index(batch, k) for k in ref.HAND_PLACED]
    assert {tri.lane_class(n) for n in lengths[len(ref.HAND_PLACED):sub["n_picked"]]} == {4, 16, 64}
    assert [int(lengths[ref.sub_index(sub, k)]) for k in ref.SUB_HAND_PLACED] == [6, 8, 8, 65]
    for name, doc in sub_recomputed["losses"].items():
        cases = doc["cases"]
        print("%s: flagged %d of %d, spread_max %.3e, iterations max %d" % (name, doc["num_near"], len(cases), doc["spread_max"], max(cs["iterations"] for cs in cases)))
        # the cap of the full batch -- at most MAX_FLAGGED_FRACTION, here one track -- holds, and the sub-batch was chosen so that none is flagged
        assert doc["num_near"] == sum(cs["near"] for cs in cases) == 0 and doc["num_near"] <= ref.MAX_FLAGGED_FRACTION * len(cases) + 1
        assert all(all(cs["fp64_agrees"]) for cs in cases)
        assert 0 < doc["spread_max"] < 1e-9
        sl = tri.track_slices(sub)
        for t, cs in enumerate(cases):      # the header's order, which the 8 sequential orders do not sample
            lane = ref.refine_fp64(sub, *sl[t], COS, MAX_SQ, loss=ref.SUB_LOSSES[name], order="lane")
            assert (lane.status, lane.termination, lane.iterations) == (cs["status"], cs["termination"], cs["iterations"]), (name, t)
        for cs in cases:
            if cs["termination"] >= 0:
                assert cs["final_cost"] <= cs["initial_cost"]


def test_hand_placed_tracks_of_the_sub_batch(sub, sub_recomputed):
    sl = tri.track_slices(sub)
    tukey, cases = sub_recomputed["losses"]["tukey"]["cases"], None

    def residual_norms(name, X):
        oc, xy = sl[ref.sub_index(sub, name)]
        return np.array([np.linalg.norm(tri._project(sub, c, X) - p) for c, p in zip(oc, xy)])
    # every observation beyond the cut at the midpoint: rho' = 0 everywhere, g = 0, the refinement stops before its first iteration
    t = ref.sub_index(sub, "all_beyond_the_tukey_cut")
    mid = ref.refine_mp(sub, *sl[t], COS, MAX_SQ, refine=False)
    assert residual_norms("all_beyond_the_tukey_cut", mid.point).min() > 12.0
    cs = tukey[t]
    assert (cs["iterations"], cs["termination"]) == (0, ref.GRADIENT_TOLERANCE) and cs["final_cost"] == cs["initial_cost"] == len(sl[t][0]) * 100.0 / 12
    assert np.array_equal(_hexpoint(cs["point"]), mid.point) and cs["status"] == mid.status
    assert sub_recomputed["losses"]["geman"]["cases"][t]["iterations"] > 0        # (a loss without a cut moves it)
    # one observation 30 px off, exact inliers: beyond the cut at the refined point it weighs nothing, so Tukey's point is more than 1e-3 from
    # Huber's and -- both run to their minimiser (SUB_CONVERGED) -- it IS the trivial loss's point of the track without that observation, within
    # the spread: in 50 digits, and in fp64 in the track's and in the kernel's order.  (At the default tolerances the runs stop at a relative
    # cost change of 1e-6, a step short of the minimiser: 2e-9 apart.)  A weight of 1e-4 leaking through the cut would move the point by 1e-6.
    t = ref.sub_index(sub, "one_beyond_the_cut")
    oc, xy = sl[t]
    oc1, xy1 = ref.without_observation(oc, xy, ref.SUB_OUTLIER_PLACE)
    centroid = tri.origin_centroid(sub, oc)
    pt = _hexpoint(tukey[t]["point"])
    norms = residual_norms("one_beyond_the_cut", pt)
    assert norms[ref.SUB_OUTLIER_PLACE] > 12.0 and np.delete(norms, ref.SUB_OUTLIER_PLACE).max() < 1e-3
    huber = ref.refine_mp(sub, oc, xy, COS, MAX_SQ, loss=ref.HUBER10).point
    assert np.linalg.norm(pt - huber) > 1e-3
    bound = 4.0 * sub_recomputed["losses"]["tukey"]["spread_max"]
    with_it, without = (_hexpoint(sub_recomputed["without_the_outlier"][k]) for k in ("tukey_with_it", "trivial"))
    worst = tri.relative_deviation(with_it, without, centroid)
    for order in (None, "lane"):
        a = ref.refine_fp64(sub, oc, xy, COS, MAX_SQ, ref.TUKEY10, ref.SUB_CONVERGED, order=order)
        b = ref.refine_fp64(sub, oc1, xy1, COS, MAX_SQ, ref.TRIVIAL, ref.SUB_CONVERGED, order=order)
        assert a.status == b.status == 0
        worst = max(worst, tri.relative_deviation(a.point, b.point, centroid), tri.relative_deviation(a.point, with_it, centroid),
                    tri.relative_deviation(b.point, without, centroid))
    print("one_beyond_the_cut: Tukey with the outlier against the trivial loss without it, worst deviation %.3e (bound %.3e)" % (worst, bound))
    assert worst <= bound
    # one observation within 1 % of the cut at the refined point
    t = ref.sub_index(sub, "at_the_cut")
    norms = residual_norms("at_the_cut", _hexpoint(tukey[t]["point"]))
    assert ((norms > 9.9) & (norms < 10.1)).sum() == 1 and tukey[t]["status"] == 0
    # five of 65 beyond the cut, in the first pass of the lanes and in the second
    t = ref.sub_index(sub, "length_65_mixed")
    norms = residual_norms("length_65_mixed", _hexpoint(tukey[t]["point"]))
    assert sorted(np.flatnonzero(norms > 10.0)) == list(ref.SUB_MIXED_PLACES) and tukey[t]["status"] == 0 and tukey[t]["iterations"] > 0


def test_losses_golden_file_matches_a_recomputation(sub_recomputed):
    with open(GOLDEN_LOSSES) as f:
        got = json.load(f)
    for k in ("sub_seed", "picks", "hand_placed"):          # ("device_measured" is what a device run printed: not compared)
        assert got[k] == sub_recomputed[k], k
    assert sorted(got["losses"]) == sorted(sub_recomputed["losses"])
    for name in got["losses"]:
        g, r = got["losses"][name], sub_recomputed["losses"][name]
        for k in ("hand_seed", "batch_seed", "orders", "mp_dps", "loss", "min_angle_degrees", "max_error_pixels", "num_near"):
            assert g[k] == r[k], (name, k)
        assert len(g["cases"]) == len(r["cases"])
        for t, (a, b) in enumerate(zip(g["cases"], r["cases"])):
            for k in ("length", "status", "n_views", "iterations", "termination", "near"):
                assert a[k] == b[k], (name, t, k, a[k], b[k])
            pa, pb = _hexpoint(a["point"]), _hexpoint(b["point"])
            assert np.max(np.abs(pa - pb)) <= 4 * 2.0 ** -53 * max(1.0, np.max(np.abs(pb))), (name, t)
            assert abs(a["final_cost"] - b["final_cost"]) <= 4 * 2.0 ** -53 * abs(b["final_cost"]), (name, t)
        assert g["spread_max"] == max(cs["spread"] for cs in g["cases"])
        assert 0.25 * r["spread_max"] <= g["spread_max"] <= 4.0 * r["spread_max"]
    for k, v in got["without_the_outlier"].items():
        pa, pb = _hexpoint(v), _hexpoint(sub_recomputed["without_the_outlier"][k])
        assert np.max(np.abs(pa - pb)) <= 4 * 2.0 ** -53 * max(1.0, np.max(np.abs(pb))), k


@pytest.mark.parametrize("defect", ["geman_unsquared", "tukey_without_half", "tukey_cut_at_a"])
def test_a_defective_loss_exceeds_the_bound_of_the_device_test(sub, sub_recomputed, defect, monkeypatch):
    """The device test's bound notices each defect: the fp64 restatement WITH it, put where the device's output goes, takes other decisions
    than the 50-digit tier or leaves 4 x spread_max on most of the sub-batch's refined tracks."""
    sound = ref._rho
    name = "geman" if defect.startswith("geman") else "tukey"

    def bad(loss, s, ops):
        r0, r1, r2 = sound(loss, s, ops)
        if loss[0] == "geman_mcclure" and defect == "geman_unsquared":
            return r0, r1 / ops.num(loss[1][1]), r2 / ops.num(loss[1][1])     # sigma2 where sigma2^2 belongs
        if loss[0] == "tukey" and defect == "tukey_without_half":
            return r0, 2 * r1, r2
        if loss[0] == "tukey" and defect == "tukey_cut_at_a" and s >= ops.num(loss[1]):     # s < a in place of s <= a^2
            return ops.num(loss[1]) ** 2 / 6, ops.num(0.0), ops.num(0.0)
        return r0, r1, r2
    monkeypatch.setattr(ref, "_rho", bad)
    doc = sub_recomputed["losses"][name]
    bound = 4.0 * doc["spread_max"]
    caught = refined = 0
    for (oc, xy), g in zip(tri.track_slices(sub), doc["cases"]):
        if g["status"] not in (0, 4, 5) or g["iterations"] == 0:
            continue
        refined += 1
        lo = ref.refine_fp64(sub, oc, xy, COS, MAX_SQ, ref.SUB_LOSSES[name], order="lane")
        flipped = (lo.status, lo.termination, lo.iterations) != (g["status"], g["termination"], g["iterations"])
        dev = tri.relative_deviation(lo.point, _hexpoint(g["point"]), tri.origin_centroid(sub, oc))
        dc = ref.relative_cost_deviation(lo.final_cost, g["final_cost"])
        caught += bool(flipped or dev > bound or dc > bound)
    print(defect, "caught on %d of %d refined tracks" % (caught, refined))
    assert refined >= 40 and caught >= 0.5 * refined


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
    # every leaf the kernel's loss_leaf_simple does not evaluate (it would run as no loss at all), a width that is not positive, a parameter
    # that is not finite: refused; Tukey and Geman-McClure with a positive width pass the checks (what comes back is the device's answer)
    nan, inf = float("nan"), float("inf")
    for node in ((_abi.LOSS_CAUCHY, 10.0), (_abi.LOSS_ARCTAN, 10.0), (_abi.LOSS_TOLERANT, 10.0, 1.0), (_abi.LOSS_LONE_HALF, 10.0), (_abi.LOSS_LTWO, 10.0, 0.5),
                 (_abi.LOSS_MAGSAC, 0.02, 9, 0), (_abi.LOSS_MAGSAC + 1, 10.0), (-1, 10.0), (_abi.LOSS_OP_COMPOSE, 10.0),
                 (_abi.LOSS_TUKEY, 0.0), (_abi.LOSS_TUKEY, -10.0), (_abi.LOSS_TUKEY, nan), (_abi.LOSS_TUKEY, inf), (_abi.LOSS_TUKEY, 10.0, nan),
                 (_abi.LOSS_GEMAN_MCCLURE, 0.0, 0.5), (_abi.LOSS_GEMAN_MCCLURE, -1.0, 0.5), (_abi.LOSS_GEMAN_MCCLURE, 10.0, nan), (_abi.LOSS_GEMAN_MCCLURE, 10.0, inf),
                 (_abi.LOSS_SOFT_L1, 0.0)):
        args, _ = _call_args(batch, loss=(node,))
        assert lib.gsfm_tracks_triangulate_refine(*args) == _abi.ERR_INVALID_ARG, node
    for node in ((_abi.LOSS_TUKEY, 10.0), (_abi.LOSS_GEMAN_MCCLURE, 10.0, 0.5), (_abi.LOSS_SOFT_L1, 10.0), (_abi.LOSS_TRIVIAL,)):
        args, _ = _call_args(batch, loss=(node,))
        assert lib.gsfm_tracks_triangulate_refine(*args) in (_abi.OK, _abi.ERR_NO_DEVICE), node
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
