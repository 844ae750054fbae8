"""Two restatements of the track triangulation as include/gsfm_tracks.h defines it (gsfm_tracks_triangulate; Theia's EstimateTrack without
the per-track refinement): plain numpy fp64 with sequential sums, and mpmath at 50 digits.  Both take one track -- the cameras (angle-axis,
position, f u v, estimated flags), the track's camera indices and pixels, cos(min angle) and the squared error bound -- and return
Result(status, point, n_views, mean_sq_err, min_cos): min_cos is the smallest pair cosine (None below 2 views), the quantity the angle test
decides on; mean_sq_err the one the gate decides on.  The fp64 version also takes a summation order (a permutation of the n estimated
observations).  Also here: the lane classes of the header, and the seeded parity batch with its hand-placed cases."""
import collections
import math

import mpmath
import numpy as np

from globalsfmpy_amd import synth

Result = collections.namedtuple("Result", "status point n_views mean_sq_err min_cos")
LEN_G4, LEN_G16 = 8, 64        # include/gsfm_tracks.h: len <= 8: 4 lanes; 9 .. 64: 16 lanes; 65 and more: 64 lanes
MIN_ANGLE_DEG, MAX_ERR_PX = 4.0, 15.0    # the reference pipeline's options


def lane_class(length):
    return 4 if length <= LEN_G4 else 16 if length <= LEN_G16 else 64


def launch_order(lengths):
    """(order, class_begin) as gsfm_tracks_launch_order defines them"""
    lengths = [int(x) for x in lengths]
    order, begin = [], [0]
    for G in (4, 16, 64):
        order += sorted((t for t in range(len(lengths)) if lane_class(lengths[t]) == G), key=lambda t: (-lengths[t], t))
        begin.append(len(order))
    return order, begin


def cos_min_angle(degrees=MIN_ANGLE_DEG):
    return math.cos(degrees * math.pi / 180.0)


# ---------------------------------------------------------------- fp64 ----
def rotation_matrix(aa):
    """Ceres' AngleAxisToRotationMatrix"""
    return synth.aa_to_matrix(np.asarray(aa, dtype=np.float64))


def triangulate_fp64(cams, obs_cam, obs_xy, c, max_sq, order=None):
    """cams: dict(rot_aa, cam_pos, intrinsics, estimated (array or None))"""
    est = cams.get("estimated")
    keep = [k for k in range(len(obs_cam)) if est is None or est[obs_cam[k]]]
    n = len(keep)
    zero = np.zeros(3)
    if n < 2:
        return Result(1, zero, n, 0.0, None)
    R = [rotation_matrix(cams["rot_aa"][obs_cam[k]]) for k in keep]
    K = [cams["intrinsics"][obs_cam[k]] for k in keep]
    O = [np.asarray(cams["cam_pos"][obs_cam[k]], dtype=np.float64) for k in keep]
    xy = [obs_xy[k] for k in keep]
    D = []
    for i in range(n):
        f, u, v = K[i]
        r = R[i].T @ np.array([(xy[i][0] - u) / f, (xy[i][1] - v) / f, 1.0])
        D.append(r / np.sqrt(r @ r))
    min_cos, passed = None, False
    for i in range(n):
        for j in range(i + 1, n):
            dot = float(D[i] @ D[j])
            if min_cos is None or dot < min_cos:       # a NaN never becomes the minimum, as it never passes the test
                min_cos = dot
            passed = passed or dot < c
    if not passed:
        return Result(2, zero, n, 0.0, min_cos)
    seq = range(n) if order is None else [int(i) for i in order]
    M, q = np.zeros((3, 3)), np.zeros(3)
    for i in seq:
        M = M + (np.eye(3) - np.outer(D[i], D[i]))
        q = q + (O[i] - D[i] * float(D[i] @ O[i]))
    p0 = M[0, 0]
    with np.errstate(all="ignore"):
        l00 = np.sqrt(p0); l10 = M[0, 1] / l00; l20 = M[0, 2] / l00
        p1 = M[1, 1] - l10 * l10
        l11 = np.sqrt(p1); l21 = (M[1, 2] - l20 * l10) / l11
        p2 = M[2, 2] - l20 * l20 - l21 * l21
        l22 = np.sqrt(p2)
    if not all(p > 0 and np.isfinite(p) for p in (p0, p1, p2)):
        return Result(3, zero, n, 0.0, min_cos)
    y0 = q[0] / l00; y1 = (q[1] - l10 * y0) / l11; y2 = (q[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
    X = np.array([x0, x1, x2])
    err, behind = 0.0, False
    with np.errstate(all="ignore"):
        for i in seq:
            p = R[i] @ (X - O[i])
            behind = behind or p[2] < 0
            f, u, v = K[i]
            err = err + ((f * p[0] / p[2] + u - xy[i][0]) ** 2 + (f * p[1] / p[2] + v - xy[i][1]) ** 2)
    mean = err / n
    return Result(4 if behind else 0 if mean < max_sq else 5, X, n, float(mean), min_cos)


# -------------------------------------------------------------- mpmath ----
MP_DPS = 50


def _mp_rotation(aa):
    mp = mpmath.mp
    w = [mp.mpf(float(x)) for x in aa]
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 > mp.mpf(float(np.finfo(np.float64).eps)):   # the branch of the fp64 routine
        th = mp.sqrt(t2)
        x, y, z = [c / th for c in w]
        c, s = mp.cos(th), mp.sin(th)
        k = 1 - c
        return [[c + x * x * k, x * y * k - z * s, y * s + x * z * k],
                [z * s + x * y * k, c + y * y * k, -x * s + y * z * k],
                [-y * s + x * z * k, x * s + y * z * k, c + z * z * k]]
    return [[mp.mpf(1), -w[2], w[1]], [w[2], mp.mpf(1), -w[0]], [-w[1], w[0], mp.mpf(1)]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def triangulate_mp(cams, obs_cam, obs_xy, c, max_sq):
    """the point comes back as fp64 (rounded from 50 digits), mean_sq_err and min_cos as mpf; c and max_sq are the fp64 thresholds"""
    with mpmath.workdps(MP_DPS):
        return _triangulate_mp(cams, obs_cam, obs_xy, c, max_sq)


def _triangulate_mp(cams, obs_cam, obs_xy, c, max_sq):
    mp = mpmath.mp
    est = cams.get("estimated")
    keep = [k for k in range(len(obs_cam)) if est is None or est[obs_cam[k]]]
    n = len(keep)
    zero = np.zeros(3)
    if n < 2:
        return Result(1, zero, n, mp.mpf(0), None)
    c, max_sq = mp.mpf(float(c)), mp.mpf(float(max_sq))
    rot_cache = {}
    R, K, O, xy, D = [], [], [], [], []
    for k in keep:
        cam = int(obs_cam[k])
        if cam not in rot_cache:
            rot_cache[cam] = _mp_rotation(cams["rot_aa"][cam])
        R.append(rot_cache[cam])
        K.append([mp.mpf(float(x)) for x in cams["intrinsics"][cam]])
        O.append([mp.mpf(float(x)) for x in cams["cam_pos"][cam]])
        xy.append([mp.mpf(float(x)) for x in obs_xy[k]])
    for i in range(n):
        f, u, v = K[i]
        ft = [(xy[i][0] - u) / f, (xy[i][1] - v) / f, mp.mpf(1)]
        r = [R[i][0][col] * ft[0] + R[i][1][col] * ft[1] + R[i][2][col] * ft[2] for col in range(3)]
        nrm = mp.sqrt(_dot(r, r))
        D.append([x / nrm for x in r])
    min_cos = None
    for i in range(n):
        for j in range(i + 1, n):
            dot = _dot(D[i], D[j])
            if min_cos is None or dot < min_cos:
                min_cos = dot
    if not min_cos < c:
        return Result(2, zero, n, mp.mpf(0), min_cos)
    M = [[mp.fsum((1 if r == col else 0) - d[r] * d[col] for d in D) for col in range(3)] for r in range(3)]
    q = [mp.fsum(o[r] - d[r] * _dot(d, o) for d, o in zip(D, O)) for r in range(3)]
    p0 = M[0][0]
    if not p0 > 0:
        return Result(3, zero, n, mp.mpf(0), min_cos)
    l00 = mp.sqrt(p0); l10 = M[0][1] / l00; l20 = M[0][2] / l00
    p1 = M[1][1] - l10 * l10
    if not p1 > 0:
        return Result(3, zero, n, mp.mpf(0), min_cos)
    l11 = mp.sqrt(p1); l21 = (M[1][2] - l20 * l10) / l11
    p2 = M[2][2] - l20 * l20 - l21 * l21
    if not p2 > 0:
        return Result(3, zero, n, mp.mpf(0), min_cos)
    l22 = mp.sqrt(p2)
    y0 = q[0] / l00; y1 = (q[1] - l10 * y0) / l11; y2 = (q[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
    X = [x0, x1, x2]
    errs, behind, singular = [], False, False
    for i in range(n):
        dlt = [X[r] - O[i][r] for r in range(3)]
        p = [_dot(R[i][r], dlt) for r in range(3)]
        behind = behind or p[2] < 0
        if p[2] == 0:
            singular = True
            continue
        f, u, v = K[i]
        errs.append((f * p[0] / p[2] + u - xy[i][0]) ** 2 + (f * p[1] / p[2] + v - xy[i][1]) ** 2)
    mean = mp.inf if singular else mp.fsum(errs) / n
    point = np.array([float(x) for x in X])
    return Result(4 if behind else 0 if mean < max_sq else 5, point, n, mean, min_cos)


def near_threshold(res, c, max_sq, rel=1e-9):
    """the decisive quantity of the 50-digit result lies within a relative `rel` of its threshold: the status may hinge on rounding"""
    if res.status in (0, 2) and res.min_cos is not None and abs(float(res.min_cos) - c) <= rel * abs(c):
        return True
    return res.status in (0, 5) and abs(float(res.mean_sq_err) - max_sq) <= rel * max_sq


def origin_centroid(cams, obs_cam):
    est = cams.get("estimated")
    keep = [k for k in range(len(obs_cam)) if est is None or est[obs_cam[k]]]
    return np.mean([cams["cam_pos"][obs_cam[k]] for k in keep], axis=0)


def relative_deviation(point, ref_point, centroid):
    return float(np.linalg.norm(np.asarray(point) - ref_point) / np.linalg.norm(ref_point - centroid))


# ----------------------------------------------------- the parity batch ----
BATCH_SEED = 5203
BATCH_LENGTHS = (2, 3, LEN_G4 - 1, LEN_G4, LEN_G4 + 1, LEN_G16 - 1, LEN_G16, LEN_G16 + 1, 129, 300)
BATCH_WEIGHTS = (0.3, 0.3, 0.08, 0.08, 0.08, 0.04, 0.04, 0.04, 0.03, 0.01)
N_RANDOM, N_CAMS = 390, 40
UNESTIMATED = (37, 38)          # cameras the random tracks see like any other: their observations are skipped at every length
TURNED = 39                     # camera 0 turned by 180 degrees about its y axis: what camera 0 sees lies behind it
HAND_PLACED = ("all_unestimated", "one_estimated_view", "pair_just_under_the_angle", "pair_just_over_the_angle", "behind_a_turned_camera",
               "one_observation_moved_200px", "unestimated_in_the_middle")


def _project(cams, cam, X):
    p = rotation_matrix(cams["rot_aa"][cam]) @ (np.asarray(X) - cams["cam_pos"][cam])
    f, u, v = cams["intrinsics"][cam]
    return np.array([f * p[0] / p[2] + u, f * p[1] / p[2] + v])


def _point_at_angle(cams, a, b, xy_a, degrees):
    """the point on camera a's ray through xy_a at which the rays of a and b meet under `degrees` (bisection on the depth)"""
    f, u, v = cams["intrinsics"][a]
    d = rotation_matrix(cams["rot_aa"][a]).T @ np.array([(xy_a[0] - u) / f, (xy_a[1] - v) / f, 1.0])
    d /= np.linalg.norm(d)
    oa, ob = cams["cam_pos"][a], cams["cam_pos"][b]

    def angle(s):
        P = oa + s * d
        w = (P - ob) / np.linalg.norm(P - ob)
        return np.degrees(np.arctan2(np.linalg.norm(np.cross(d, w)), float(d @ w)))
    lo, hi = 1.0, 1e4                       # the angle falls with the depth
    assert angle(lo) > degrees > angle(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if angle(mid) > degrees else (lo, mid)
    return oa + 0.5 * (lo + hi) * d


def make_batch():
    """The parity batch as flat arrays: N_RANDOM tracks of synth.make_tracks over the first 39 cameras (0.5 px noise, 1 % gross outliers),
    then the hand-placed tracks, in the order of HAND_PLACED."""
    g = synth.make_tracks(N_CAMS - 1, N_RANDOM, BATCH_SEED, lengths=BATCH_LENGTHS, length_weights=BATCH_WEIGHTS, noise_px=0.5, outlier_frac=0.01)
    turn = np.diag([-1.0, 1.0, -1.0]) @ rotation_matrix(g["rot_aa"][0])
    cams = {"rot_aa": np.vstack([g["rot_aa"], synth.quat_to_aa(synth.matrix_to_quat(turn[None]))]), "cam_pos": np.vstack([g["cam_pos"], g["cam_pos"][:1]]),
            "intrinsics": np.vstack([g["intrinsics"], g["intrinsics"][:1]])}
    est = np.ones(N_CAMS, dtype=np.uint8)
    est[list(UNESTIMATED)] = 0
    cams["estimated"] = est
    P = np.array([0.4, -0.3, 0.6])
    tracks = []

    def seen(cam_list, X=P):
        return [(c, _project(cams, c, X)) for c in cam_list]
    tracks.append(seen(UNESTIMATED))
    tracks.append(seen((UNESTIMATED[0], 5, UNESTIMATED[1])))
    # camera 10 and its nearest estimated neighbour that looks the same way: a far point lies in front of both
    axis = [rotation_matrix(cams["rot_aa"][k])[2] for k in range(N_CAMS - 1)]
    near = min((k for k in range(N_CAMS - 1) if k != 10 and est[k] and axis[k] @ axis[10] > 0.8), key=lambda k: np.linalg.norm(cams["cam_pos"][k] - cams["cam_pos"][10]))
    for deg in (MIN_ANGLE_DEG - 1e-4, MIN_ANGLE_DEG + 1e-4):
        xy_a = cams["intrinsics"][10][1:] + np.array([31.0, -17.0])
        Q = _point_at_angle(cams, 10, near, xy_a, deg)
        assert all((rotation_matrix(cams["rot_aa"][k]) @ (Q - cams["cam_pos"][k]))[2] > 1.0 for k in (10, near))
        tracks.append([(10, xy_a), (near, _project(cams, near, Q))])
    x0 = _project(cams, 0, P)                 # camera 0's pixel, mirrored in y: the same line through P for the turned camera
    tracks.append([(TURNED, np.array([x0[0], 2.0 * cams["intrinsics"][0][2] - x0[1]])), (5, _project(cams, 5, P))])
    moved = seen((1, 2, 3))
    moved[1] = (2, moved[1][1] + np.array([200.0, 0.0]))
    tracks.append(moved)
    tracks.append(seen((4, UNESTIMATED[0], 6, UNESTIMATED[1], 8)))
    assert len(tracks) == len(HAND_PLACED)
    obs_cam = np.concatenate([g["obs_cam"], np.array([c for t in tracks for c, _ in t], dtype=np.uint32)])
    obs_xy = np.vstack([g["obs_xy"], np.array([xy for t in tracks for _, xy in t])])
    ptr = np.concatenate([g["track_ptr"], g["track_ptr"][-1] + np.cumsum([len(t) for t in tracks]).astype(np.uint64)]).astype(np.uint64)
    return {"n_cams": N_CAMS, "rot_aa": np.ascontiguousarray(cams["rot_aa"]), "cam_pos": np.ascontiguousarray(cams["cam_pos"]),
            "intrinsics": np.ascontiguousarray(cams["intrinsics"]), "estimated": est, "track_ptr": ptr, "obs_cam": obs_cam, "obs_xy": obs_xy,
            "n_random": N_RANDOM}


def track_slices(batch):
    ptr = batch["track_ptr"].astype(np.int64)
    return [(batch["obs_cam"][ptr[t]:ptr[t + 1]], batch["obs_xy"][ptr[t]:ptr[t + 1]]) for t in range(len(ptr) - 1)]


# ------------------------------------------------------ the golden file ----
ORDERS = 8


def compute_golden(batch=None):
    """Per track of the batch: the 50-digit result and the fp64 restatement's worst relative deviation from it over ORDERS summation orders
    (the given order first, then seeded permutations)."""
    batch = batch or make_batch()
    c, max_sq = cos_min_angle(), MAX_ERR_PX ** 2
    cases = []
    for t, (oc, xy) in enumerate(track_slices(batch)):
        hp = triangulate_mp(batch, oc, xy, c, max_sq)
        case = {"length": int(len(oc)), "status": hp.status, "n_views": hp.n_views, "point": [float(x).hex() for x in hp.point],
                "min_cos": None if hp.min_cos is None else float(hp.min_cos), "mean_sq_err": float(hp.mean_sq_err),
                "near_threshold": bool(near_threshold(hp, c, max_sq)), "spread": 0.0, "fp64_status": []}
        if hp.status in (0, 4, 5):
            rng = np.random.Generator(np.random.PCG64(BATCH_SEED + 50000 + t))
            centroid = origin_centroid(batch, oc)
            for k in range(ORDERS):
                lo = triangulate_fp64(batch, oc, xy, c, max_sq, order=None if k == 0 else rng.permutation(hp.n_views))
                case["fp64_status"].append(lo.status)
                case["spread"] = max(case["spread"], relative_deviation(lo.point, hp.point, centroid))
        else:
            case["fp64_status"].append(triangulate_fp64(batch, oc, xy, c, max_sq).status)
        cases.append(case)
    return {"batch_seed": BATCH_SEED, "orders": ORDERS, "mp_dps": MP_DPS, "min_angle_degrees": MIN_ANGLE_DEG, "max_error_pixels": MAX_ERR_PX,
            "num_near_threshold": sum(cs["near_threshold"] for cs in cases), "spread_max": max(cs["spread"] for cs in cases), "cases": cases}
