"""Two restatements of the outlier rule as include/gsfm_tracks.h defines it (gsfm_tracks_outlier_tracks; Theia's
SetOutlierTracksToUnestimated): plain numpy fp64 with sequential sums, and mpmath at 50 digits.  Both take one track that is estimated on
input -- the cameras (angle-axis, position, f u v, estimated flags), the track's camera indices and pixels, its point, cos(min angle) and
the squared error bound -- and return Result(status, n_views, mean_sq_err, min_cos): min_cos is the smallest pair cosine of the rays from
the camera centres to the point (None when no pair compares: fewer than 2 views, or NaN rays), the quantity the angle test decides on.  The
fp64 version also takes a summation order (a permutation of the n estimated observations).  Also here: the seeded parity batch with its
hand-placed cases, and the golden file's content."""
import collections
import functools
import json
import math
import os

import mpmath
import numpy as np

import triangulation_reference as tri
from triangulation_reference import MP_DPS, _dot, _mp_rotation, rotation_matrix

Result = collections.namedtuple("Result", "status n_views mean_sq_err min_cos")
MAX_ERR_PX, MIN_ANGLE_DEG = 5.0, 4.0     # Theia's defaults (max_reprojection_error_in_pixels, min_triangulation_angle_degrees)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cos_min_angle(degrees=MIN_ANGLE_DEG):
    return math.cos(degrees * math.pi / 180.0)


def _kept(cams, obs_cam):
    est = cams.get("estimated")
    return [k for k in range(len(obs_cam)) if est is None or est[obs_cam[k]]]


# ---------------------------------------------------------------- fp64 ----
def outlier_fp64(cams, obs_cam, obs_xy, point, c, max_sq, order=None):
    keep = _kept(cams, obs_cam)
    n = len(keep)
    X = np.asarray(point, dtype=np.float64)
    R = [rotation_matrix(cams["rot_aa"][obs_cam[k]]) for k in keep]
    K = [cams["intrinsics"][obs_cam[k]] for k in keep]
    O = [np.asarray(cams["cam_pos"][obs_cam[k]], dtype=np.float64) for k in keep]
    xy = [obs_xy[k] for k in keep]
    seq = range(n) if order is None else [int(i) for i in order]
    err, behind = 0.0, False
    with np.errstate(all="ignore"):
        for i in seq:
            p = R[i] @ (X - O[i])
            behind = behind or p[2] < 0
            f, u, v = K[i]
            err = err + ((f * p[0] / p[2] + u - xy[i][0]) ** 2 + (f * p[1] / p[2] + v - xy[i][1]) ** 2)
        mean = float(np.float64(err) / np.float64(n))
        D = np.zeros((n, 3))
        for i in range(n):
            w = X - O[i]
            D[i] = w / np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        min_cos = None
        if n >= 2:
            G = D @ D.T
            pair = G[np.triu_indices(n, 1)]
            pair = pair[~np.isnan(pair)]
            min_cos = float(pair.min()) if pair.size else None
    if behind:
        return Result(2, n, mean, min_cos)
    if mean > max_sq:
        return Result(3, n, mean, min_cos)
    return Result(0 if min_cos is not None and min_cos < c else 4, n, mean, min_cos)


# -------------------------------------------------------------- mpmath ----
def outlier_mp(cams, obs_cam, obs_xy, point, c, max_sq):
    """mean_sq_err and min_cos come back as mpf (mean: nan where it is 0 / 0, +inf where a p_z is 0 beside a finite numerator)"""
    with mpmath.workdps(MP_DPS):
        return _outlier_mp(cams, obs_cam, obs_xy, point, c, max_sq)


def _outlier_mp(cams, obs_cam, obs_xy, point, c, max_sq):
    mp = mpmath.mp
    keep = _kept(cams, obs_cam)
    n = len(keep)
    c, max_sq = mp.mpf(float(c)), mp.mpf(float(max_sq))
    X = [mp.mpf(float(x)) for x in point]
    rot_cache = {}
    errs, D, behind, nan_mean, inf_mean = [], [], False, n == 0, False
    for k in keep:
        cam = int(obs_cam[k])
        if cam not in rot_cache:
            rot_cache[cam] = _mp_rotation(cams["rot_aa"][cam])
        R = rot_cache[cam]
        f, u, v = [mp.mpf(float(x)) for x in cams["intrinsics"][cam]]
        o = [mp.mpf(float(x)) for x in cams["cam_pos"][cam]]
        xy = [mp.mpf(float(x)) for x in obs_xy[k]]
        w = [X[r] - o[r] for r in range(3)]
        p = [_dot(R[r], w) for r in range(3)]
        behind = behind or p[2] < 0
        if p[2] == 0:                                # IEEE: 0 / 0 is NaN, anything else / 0 is infinite
            if p[0] == 0 or p[1] == 0:
                nan_mean = True
            else:
                inf_mean = True
        else:
            errs.append((f * p[0] / p[2] + u - xy[0]) ** 2 + (f * p[1] / p[2] + v - xy[1]) ** 2)
        nrm = mp.sqrt(_dot(w, w))
        D.append(None if nrm == 0 else [x / nrm for x in w])
    mean = mp.nan if nan_mean else mp.inf if inf_mean else mp.fsum(errs) / n
    min_cos = None
    for i in range(n):
        for j in range(i + 1, n):
            if D[i] is None or D[j] is None:
                continue
            dot = _dot(D[i], D[j])
            if min_cos is None or dot < min_cos:
                min_cos = dot
    if behind:
        return Result(2, n, mean, min_cos)
    if not nan_mean and mean > max_sq:
        return Result(3, n, mean, min_cos)
    return Result(0 if min_cos is not None and min_cos < c else 4, n, mean, min_cos)


def near_threshold(res, c, max_sq, rel=1e-9):
    """the decisive quantity of the 50-digit result lies within a relative `rel` of its threshold: the status may hinge on rounding
    (triangulation_reference.near_threshold's rule for this entry's two thresholds)"""
    if res.status in (0, 4) and res.min_cos is not None and abs(float(res.min_cos) - c) <= rel * abs(c):
        return True
    mean = float(res.mean_sq_err)
    return res.status in (0, 3, 4) and math.isfinite(mean) and abs(mean - max_sq) <= rel * max_sq


# ----------------------------------------------------- the parity batch ----
BATCH_SEED = 9127
NARROW_LENGTHS = (7, 8, 9, 63, 64, 65, 129, 300)     # tracks built for status 4: both sides of every lane-class edge
HAND_PLACED = ("not_estimated_on_input", "all_views_unestimated", "one_estimated_view", "pair_just_under_the_angle", "pair_just_over_the_angle",
               "behind_the_turned_camera", "mean_just_under_16", "mean_just_over_16", "point_at_a_camera_centre")
HAND_STATUS = (1, 4, 4, 4, 0, 2, 0, 3, 4)
MEAN16_BOUND_PX = 4.0                                # the two mean cases run in a call of their own with this bound: 16 = 4^2


def _exact_projection(cams, cam, X):
    """the pixel of X in camera `cam`, rounded from 50 digits"""
    with mpmath.workdps(MP_DPS):
        mp = mpmath.mp
        R = _mp_rotation(cams["rot_aa"][cam])
        w = [mp.mpf(float(X[r])) - mp.mpf(float(cams["cam_pos"][cam][r])) for r in range(3)]
        p = [_dot(R[r], w) for r in range(3)]
        f, u, v = [mp.mpf(float(x)) for x in cams["intrinsics"][cam]]
        return np.array([float(f * p[0] / p[2] + u), float(f * p[1] / p[2] + v)])


@functools.lru_cache(maxsize=None)
def make_batch():
    """The parity batch as flat arrays (the keys of triangulation_reference.make_batch() plus points, point_estimated, kind, bound_px).
    Cameras: those of the triangulation batch, the two unestimated ones and the turned one included.
      random   that batch's N_RANDOM tracks (lengths 2, 3, 7, 8, 9, 63, 64, 65, 129, 300) with the 50-digit midpoints of
               tests/golden/triangulation_spread.json as their points (zero where the triangulation gave none).  A seeded quarter is displaced:
               mirrored through the centre of the track's first estimated camera (behind it: status 2), or shifted sideways by a tenth of its
               distance from the cameras' centroid (status 3).
      narrow   per length of NARROW_LENGTHS a track over the estimated cameras that look along the mean viewing direction, its point moved
               out along that direction until every pair of rays meets under less than a degree, its pixels the projections of the moved point
               plus 0.5 px of seeded noise.  The rule tests the reprojection error first, so a status 4 needs pixels that agree with the point:
               displacing a random track's point alone ends in status 2 or 3.
      hand     the cases of HAND_PLACED.
    Do not modify the returned arrays."""
    b = tri.make_batch()
    cams = {k: b[k] for k in ("rot_aa", "cam_pos", "intrinsics", "estimated")}
    est = b["estimated"]
    with open(os.path.join(GOLDEN_DIR, "triangulation_spread.json")) as f:
        spread = json.load(f)
    assert spread["batch_seed"] == tri.BATCH_SEED
    n_random = b["n_random"]
    ptr = b["track_ptr"].astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(BATCH_SEED))
    centroid = b["cam_pos"][est != 0].mean(axis=0)
    tracks, points, kinds = [], [], []
    for t in range(n_random):
        oc, xy = b["obs_cam"][ptr[t]:ptr[t + 1]], b["obs_xy"][ptr[t]:ptr[t + 1]]
        X = np.array([float.fromhex(h) for h in spread["cases"][t]["point"]])
        kind = "random"
        first = next((int(c) for c in oc if est[c]), None)
        draw, side = rng.random(), rng.standard_normal(3)
        if draw < 0.25 and first is not None and X.any():
            if draw < 0.125:
                X = 2.0 * b["cam_pos"][first] - X
                kind = "mirrored"
            else:
                X = X + 0.1 * np.linalg.norm(X - centroid) * side / np.linalg.norm(side)
                kind = "shifted"
        tracks.append(list(zip(oc, xy)))
        points.append(X)
        kinds.append(kind)
    # the narrow tracks
    axis = np.array([rotation_matrix(b["rot_aa"][k])[2] for k in range(b["n_cams"])])
    usable = [k for k in range(b["n_cams"]) if est[k] and k != tri.TURNED]
    u = axis[usable].mean(axis=0)
    u /= np.linalg.norm(u)
    group = [k for k in usable if axis[k] @ u > 0.5]
    assert len(group) >= 7, len(group)
    spread_m = max(np.linalg.norm(b["cam_pos"][k] - centroid) for k in group)
    far = centroid + 400.0 * spread_m * u                          # every pair of rays within 2 atan(1 / 400) < 0.3 degrees
    for L in NARROW_LENGTHS:
        seen = [group[i % len(group)] for i in range(L)]
        tracks.append([(c, _exact_projection(cams, c, far) + 0.5 * rng.standard_normal(2)) for c in seen])
        points.append(far.copy())
        kinds.append("narrow")
    # the hand-placed cases
    P = np.array([0.4, -0.3, 0.6])
    hb = ptr[n_random:]                                           # the triangulation batch's own hand-placed tracks
    hand = lambda i: list(zip(b["obs_cam"][hb[i]:hb[i + 1]], b["obs_xy"][hb[i]:hb[i + 1]]))   # noqa: E731

    def seen_from(cam_list, X, offset=(0.0, 0.0)):
        return [(c, _exact_projection(cams, c, X) + np.asarray(offset)) for c in cam_list]
    tracks.append(seen_from((1, 2, 3), P)); points.append(P)                                      # not estimated on input
    tracks.append(hand(0)); points.append(P)                                                      # all views unestimated: n = 0
    tracks.append(hand(1)); points.append(P)                                                      # one estimated view
    near = min((k for k in usable if k != 10 and axis[k] @ axis[10] > 0.8), key=lambda k: np.linalg.norm(b["cam_pos"][k] - b["cam_pos"][10]))
    for deg in (MIN_ANGLE_DEG - 1e-4, MIN_ANGLE_DEG + 1e-4):                                      # the angle AT THE POINT
        xy_a = b["intrinsics"][10][1:] + np.array([31.0, -17.0])
        Q = tri._point_at_angle(cams, 10, near, xy_a, deg)
        tracks.append(seen_from((10, near), Q)); points.append(Q)
    tracks.append(seen_from((tri.TURNED, 5), P)); points.append(P)                                # camera 0 sees P, so P lies behind the turned one
    for scale in (1.0 - 1e-6, 1.0 + 1e-6):                                                        # every view off by the same pixel offset: mean = |offset|^2
        off = math.sqrt(16.0 * scale / 2.0)
        tracks.append(seen_from((1, 2, 3), P, (off, off))); points.append(P)
    # exactly at camera 4's centre, which the other view has in front of it: a NaN mean, no p_z < 0, and one ray that compares
    other = next(k for k in usable if k != 4 and (rotation_matrix(b["rot_aa"][k]) @ (b["cam_pos"][4] - b["cam_pos"][k]))[2] > 0.1)
    tracks.append(seen_from((4, other), P)); points.append(b["cam_pos"][4].copy())
    kinds += ["hand:" + name for name in HAND_PLACED]
    assert len(tracks) == len(points) == len(kinds)
    point_estimated = np.ones(len(tracks), dtype=np.uint8)
    point_estimated[kinds.index("hand:not_estimated_on_input")] = 0
    bound = np.full(len(tracks), MAX_ERR_PX)
    for name in ("mean_just_under_16", "mean_just_over_16"):
        bound[kinds.index("hand:" + name)] = MEAN16_BOUND_PX
    out = {k: b[k] for k in ("n_cams", "rot_aa", "cam_pos", "intrinsics", "estimated")}
    out["obs_cam"] = np.array([c for t in tracks for c, _ in t], dtype=np.uint32)
    out["obs_xy"] = np.ascontiguousarray(np.array([xy for t in tracks for _, xy in t], dtype=np.float64).reshape(-1, 2))
    out["track_ptr"] = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint64)
    out["points"] = np.ascontiguousarray(np.array(points, dtype=np.float64))
    out["point_estimated"] = point_estimated
    out["kind"] = kinds
    out["bound_px"] = bound
    return out


def hand_index(batch, name):
    return batch["kind"].index("hand:" + name)


def track_slices(batch):
    ptr = batch["track_ptr"].astype(np.int64)
    return [(batch["obs_cam"][ptr[t]:ptr[t + 1]], batch["obs_xy"][ptr[t]:ptr[t + 1]]) for t in range(len(ptr) - 1)]


# ------------------------------------------------------ the golden file ----
ORDERS = 8


def _num(x):
    x = float(x)
    return x if math.isfinite(x) else repr(x)        # JSON has no nan / inf


@functools.lru_cache(maxsize=None)
def reference_results():
    """per track of the batch the 50-digit Result (None for the track that is not estimated on input), computed once per process"""
    batch = make_batch()
    c = cos_min_angle()
    return tuple(outlier_mp(batch, oc, xy, batch["points"][t], c, batch["bound_px"][t] ** 2) if batch["point_estimated"][t] else None
                 for t, (oc, xy) in enumerate(track_slices(batch)))


def compute_golden():
    """Per track of the batch: the 50-digit result and the fp64 restatement's worst relative deviation of the mean from it over ORDERS
    summation orders (the given order first, then seeded permutations), with the fp64 status of every order."""
    batch = make_batch()
    c = cos_min_angle()
    cases = []
    for t, ((oc, xy), hp) in enumerate(zip(track_slices(batch), reference_results())):
        if hp is None:
            cases.append({"kind": batch["kind"][t], "length": int(len(oc)), "status": 1, "n_views": 0, "mean_sq_err": 0.0, "min_cos": None,
                          "near_threshold": False, "spread": 0.0, "fp64_status": []})
            continue
        max_sq = batch["bound_px"][t] ** 2
        case = {"kind": batch["kind"][t], "length": int(len(oc)), "status": hp.status, "n_views": hp.n_views, "mean_sq_err": _num(hp.mean_sq_err),
                "min_cos": None if hp.min_cos is None else float(hp.min_cos), "near_threshold": bool(near_threshold(hp, c, max_sq)),
                "spread": 0.0, "fp64_status": []}
        rng = np.random.Generator(np.random.PCG64(BATCH_SEED + 50000 + t))
        for k in range(ORDERS):
            lo = outlier_fp64(batch, oc, xy, batch["points"][t], c, max_sq, order=None if k == 0 else rng.permutation(hp.n_views))
            case["fp64_status"].append(lo.status)
            ref = float(hp.mean_sq_err)
            if math.isfinite(ref):
                case["spread"] = max(case["spread"], abs(lo.mean_sq_err - ref) / max(1.0, abs(ref)))
        cases.append(case)
    return {"batch_seed": BATCH_SEED, "orders": ORDERS, "mp_dps": MP_DPS, "min_angle_degrees": MIN_ANGLE_DEG, "max_error_pixels": MAX_ERR_PX,
            "num_near_threshold": sum(cs["near_threshold"] for cs in cases), "spread_max": max(cs["spread"] for cs in cases), "cases": cases}
