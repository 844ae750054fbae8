"""Two restatements of the track triangulation with the per-track refinement as include/gsfm_tracks.h defines it
(gsfm_tracks_triangulate_refine; Theia's EstimateTrack with BundleAdjustTrack): numpy fp64 and mpmath at 50 digits, ONE text run on two
number types.  Both take one track and return Result(status, point, n_views, mean_sq_err, iterations, termination, initial_cost,
final_cost, near): `near` says that some accept / stop / gate quantity came within a relative 1e-9 of its threshold, so that the decision
may hinge on rounding.  The fp64 version takes a summation order: None (the track's order), a permutation of the estimated observations,
or "lane" -- the header's order (lane stride G, then the xor butterfly).  Also here: the parity batch, triangulation_reference.make_batch()
plus hand-placed tracks, and the golden file's content."""
import collections
import json
import math

import mpmath
import numpy as np

import triangulation_reference as tri

Result = collections.namedtuple("Result", "status point n_views mean_sq_err iterations termination initial_cost final_cost near")
FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, PARAMETER_TOLERANCE, NO_CONVERGENCE, FAILURE = range(5)     # gsfm_rot_termination
OPTIONS = {"max_num_iterations": 100, "function_tolerance": 1e-6, "gradient_tolerance": 1e-10, "parameter_tolerance": 1e-8,
           "min_relative_decrease": 1e-3, "initial_radius": 1e4, "max_radius": 1e12, "min_radius": 1e-32}
TRIVIAL, HUBER10 = ("trivial", 0.0), ("huber", 10.0)     # Theia's TRIVIAL and the reference YAML's HUBER with its width
SOFTL1_10, TUKEY10, GEMAN10 = ("softl1", 10.0), ("tukey", 10.0), ("geman_mcclure", (10.0, 0.5))     # the other leaves the entry takes
NEAR_REL = 1e-9
DBL_MIN = 2.2250738585072014e-308


class _Fp64:
    mp = False

    @staticmethod
    def num(x):
        return np.float64(x)

    @staticmethod
    def sqrt(x):
        return np.sqrt(x)

    @staticmethod
    def finite(x):
        return bool(np.isfinite(x))

    @staticmethod
    def rotation(aa):
        return [[np.float64(v) for v in row] for row in tri.rotation_matrix(aa)]


class _Mp:
    mp = True

    @staticmethod
    def num(x):
        return mpmath.mpf(float(x))

    @staticmethod
    def sqrt(x):
        return mpmath.sqrt(x) if x >= 0 else mpmath.nan

    @staticmethod
    def finite(x):
        return bool(mpmath.isfinite(x))

    @staticmethod
    def rotation(aa):
        return tri._mp_rotation(aa)


def _total(terms, places, length, order, ops):
    """the sum of `terms` (a list per estimated observation, `places` its place in the track) in the given order"""
    width = len(terms[0]) if terms else 0
    zero = [ops.num(0.0)] * width
    if ops.mp:
        return [mpmath.fsum(t[c] for t in terms) for c in range(width)]
    if isinstance(order, str):
        assert order == "lane"
        G = tri.lane_class(length)
        lanes = [list(zero) for _ in range(G)]
        for t, k in zip(terms, places):                  # places ascend: lane l adds the places l, l + G, ... in that order
            lanes[k % G] = [a + b for a, b in zip(lanes[k % G], t)]
        off = G // 2
        while off:
            lanes = [[a + b for a, b in zip(lanes[l], lanes[l ^ off])] for l in range(G)]
            off //= 2
        return lanes[0]
    acc = list(zero)
    for i in (range(len(terms)) if order is None else [int(i) for i in order]):
        acc = [a + b for a, b in zip(acc, terms[i])]
    return acc


def _div(a, b, ops):
    if ops.mp and b == 0:
        return mpmath.nan if a == 0 else mpmath.inf * a
    return a / b


def _cholesky_solve(M, q, ops):
    """the 3 x 3 Cholesky of the header: M as xx xy xz yy yz zz; None when a pivot is not positive or not finite"""
    p0 = M[0]
    if not (p0 > 0 and ops.finite(p0)):
        return None
    l00 = ops.sqrt(p0); l10 = M[1] / l00; l20 = M[2] / l00
    p1 = M[3] - l10 * l10
    if not (p1 > 0 and ops.finite(p1)):
        return None
    l11 = ops.sqrt(p1); l21 = (M[4] - l20 * l10) / l11
    p2 = M[5] - l20 * l20 - l21 * l21
    if not (p2 > 0 and ops.finite(p2)):
        return None
    l22 = ops.sqrt(p2)
    y0 = q[0] / l00; y1 = (q[1] - l10 * y0) / l11; y2 = (q[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return [x0, x1, x2]


def _rho(loss, s, ops):
    """(rho, rho', rho'') at s: Ceres' formulas as position_hp_reference.loss_rho states them; Geman-McClure's second parameter is
    loss_functions.GemanMcClureLoss's sigma2 and enters as it stands"""
    kind, a = loss
    one, zero = ops.num(1.0), ops.num(0.0)
    if kind == "trivial":
        return s, one, zero
    params = tuple(a) if isinstance(a, (tuple, list)) else (a,)
    a = ops.num(params[0])
    b = a * a
    if kind == "huber":
        if s > b:
            r = ops.sqrt(s)
            r1 = max(a / r, ops.num(DBL_MIN))
            return 2 * a * r - b, r1, -r1 / (2 * s)
        return s, one, zero
    if kind == "softl1":
        sm = 1 + s / b
        tmp = ops.sqrt(sm)
        r1 = max(1 / tmp, ops.num(DBL_MIN))
        return 2 * b * (tmp - 1), r1, -(r1 / b) / (2 * sm)
    if kind == "tukey":
        if s <= b:
            v = 1 - s / b
            return b / 6 * (1 - v * v * v), v * v / 2, -v / b
        return b / 6, zero, zero
    assert kind == "geman_mcclure"
    g2 = ops.num(params[1])
    t = s / b + g2
    return b * g2 * s / (2 * (s + b * g2)), g2 * g2 / (2 * t * t), -(g2 * g2) / (b * t * t * t)


class _Track:
    """one track's estimated observations on a number type"""

    def __init__(self, cams, obs_cam, obs_xy, ops):
        est = cams.get("estimated")
        self.places = [k for k in range(len(obs_cam)) if est is None or est[obs_cam[k]]]
        self.length, self.n, self.ops = len(obs_cam), len(self.places), ops
        cache = {}
        self.R, self.K, self.O, self.xy = [], [], [], []
        for k in self.places:
            cam = int(obs_cam[k])
            if cam not in cache:
                cache[cam] = ops.rotation(cams["rot_aa"][cam])
            self.R.append(cache[cam])
            self.K.append([ops.num(x) for x in cams["intrinsics"][cam]])
            self.O.append([ops.num(x) for x in cams["cam_pos"][cam]])
            self.xy.append([ops.num(x) for x in obs_xy[k]])

    def project(self, i, X):
        R, O = self.R[i], self.O[i]
        v = [X[c] - O[c] for c in range(3)]
        return [R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] for r in range(3)]

    def residual(self, i, p):
        f, u, v = self.K[i]
        return [_div(f * p[0], p[2], self.ops) + u - self.xy[i][0], _div(f * p[1], p[2], self.ops) + v - self.xy[i][1]]

    def passes(self, X, loss, order):
        """the ten sums of a pass: J^T J (xx xy xz yy yz zz), g (x y z), cost"""
        ops, terms = self.ops, []
        for i in range(self.n):
            p = self.project(i, X)
            e = self.residual(i, p)
            s = e[0] * e[0] + e[1] * e[1]
            if not ops.finite(s):
                terms.append([ops.num(float("nan"))] * 10)
                continue
            r0, r1, r2 = _rho(loss, s, ops)
            sr = ops.sqrt(r1)
            if s == 0 or r2 <= 0:
                scaling, asn = sr, ops.num(0.0)
            else:
                alpha = 1 - ops.sqrt(1 + 2 * s * r2 / r1)
                scaling, asn = sr / (1 - alpha), alpha / s
            f, R = self.K[i][0], self.R[i]
            fz, ax, ay = f / p[2], p[0] / p[2], p[1] / p[2]
            J0 = [fz * (R[0][j] - ax * R[2][j]) for j in range(3)]
            J1 = [fz * (R[1][j] - ay * R[2][j]) for j in range(3)]
            if asn != 0:
                for j in range(3):
                    t = asn * (e[0] * J0[j] + e[1] * J1[j])
                    J0[j] -= e[0] * t; J1[j] -= e[1] * t
            J0 = [x * sr for x in J0]; J1 = [x * sr for x in J1]
            q0, q1 = scaling * e[0], scaling * e[1]
            terms.append([J0[0] * J0[0] + J1[0] * J1[0], J0[0] * J0[1] + J1[0] * J1[1], J0[0] * J0[2] + J1[0] * J1[2],
                          J0[1] * J0[1] + J1[1] * J1[1], J0[1] * J0[2] + J1[1] * J1[2], J0[2] * J0[2] + J1[2] * J1[2],
                          J0[0] * q0 + J1[0] * q1, J0[1] * q0 + J1[1] * q1, J0[2] * q0 + J1[2] * q1, r0 / 2])
        return _total(terms, self.places, self.length, order, ops)


class _Near:
    def __init__(self):
        self.flag = False

    def __call__(self, q, thr):
        """records a quantity that comes within NEAR_REL (relative) of the threshold it is compared with"""
        q, thr = float(q), float(thr)
        if math.isfinite(q) and thr != 0.0 and abs(q - thr) <= NEAR_REL * abs(thr):
            self.flag = True


def _refine(cams, obs_cam, obs_xy, c, max_sq, loss, options, order, ops, refine=True):
    o = dict(OPTIONS, **(options or {}))
    num = ops.num
    near = _Near()
    tk = _Track(cams, obs_cam, obs_xy, ops)
    n = tk.n
    zero3 = np.zeros(3)

    def out(status, X, mean, it=0, term=-1, c0=0.0, c1=0.0):
        return Result(status, zero3 if X is None else np.array([float(x) for x in X]), n, mean, it, term, c0, c1, near.flag)
    if n < 2:
        return out(1, None, num(0.0))
    # ---- steps 1 to 4 ----
    D = []
    for i in range(n):
        f, u, v = tk.K[i]
        ft = [(tk.xy[i][0] - u) / f, (tk.xy[i][1] - v) / f, num(1.0)]
        R = tk.R[i]
        r = [R[0][col] * ft[0] + R[1][col] * ft[1] + R[2][col] * ft[2] for col in range(3)]
        nrm = ops.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        D.append([x / nrm for x in r])
    min_cos = min(D[i][0] * D[j][0] + D[i][1] * D[j][1] + D[i][2] * D[j][2] for i in range(n) for j in range(i + 1, n))
    near(min_cos, c)
    if not min_cos < num(c):
        return out(2, None, num(0.0))
    terms = []
    for d, og in zip(D, tk.O):
        dox = d[0] * og[0] + d[1] * og[1] + d[2] * og[2]
        terms.append([1 - d[0] * d[0], -(d[0] * d[1]), -(d[0] * d[2]), 1 - d[1] * d[1], -(d[1] * d[2]), 1 - d[2] * d[2],
                      og[0] - d[0] * dox, og[1] - d[1] * dox, og[2] - d[2] * dox])
    S9 = _total(terms, tk.places, tk.length, order, ops)
    X = _cholesky_solve(S9[:6], S9[6:], ops)
    if X is None:
        return out(3, None, num(0.0))
    # ---- the refinement ----
    it, term, c0, x_cost = 0, -1, 0.0, num(0.0)
    if refine:
        S = tk.passes(X, loss, order)
        x_cost = c0 = S[9]
        gmax = max(abs(S[6]), abs(S[7]), abs(S[8]))
        sc = [1 / (1 + ops.sqrt(S[k])) for k in (0, 3, 5)] if ops.finite(S[0] + S[3] + S[5]) else [num(1.0)] * 3
        radius, factor, invalid, last_ok = num(o["initial_radius"]), num(2.0), 0, False
        gtol, ptol, ftol = num(o["gradient_tolerance"]), num(o["parameter_tolerance"]), num(o["function_tolerance"])
        near(gmax, gtol)
        if not ops.finite(x_cost):
            term = FAILURE
        elif gmax <= gtol:
            term = GRADIENT_TOLERANCE
        elif o["max_num_iterations"] <= 0:
            term = NO_CONVERGENCE
        while term < 0:
            it += 1
            A = [S[0] * sc[0] * sc[0], S[1] * sc[0] * sc[1], S[2] * sc[0] * sc[2], S[3] * sc[1] * sc[1], S[4] * sc[1] * sc[2], S[5] * sc[2] * sc[2]]
            for k in (0, 3, 5):
                A[k] = A[k] + min(max(A[k], num(1e-6)), num(1e32)) / radius
            e = _cholesky_solve(A, [-(S[6] * sc[0]), -(S[7] * sc[1]), -(S[8] * sc[2])], ops)
            valid, cand = e is not None, None
            if valid:
                d = [e[k] * sc[k] for k in range(3)]
                Hd = [S[0] * d[0] + S[1] * d[1] + S[2] * d[2], S[1] * d[0] + S[3] * d[1] + S[4] * d[2], S[2] * d[0] + S[4] * d[1] + S[5] * d[2]]
                model = -(d[0] * S[6] + d[1] * S[7] + d[2] * S[8]) - (d[0] * Hd[0] + d[1] * Hd[1] + d[2] * Hd[2]) / 2
                valid = ops.finite(model) and model > 0
            if valid:
                Xt = [X[k] + d[k] for k in range(3)]
                St = tk.passes(Xt, loss, order)
                cand = St[9]
                valid = ops.finite(cand)
            if not valid:
                invalid += 1
                if invalid >= 5:
                    term = FAILURE
                else:
                    radius = radius / factor; factor = factor * 2
                last_ok = False
            else:
                invalid = 0
                step_norm = ops.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                x_norm = ops.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
                change = x_cost - cand
                near(step_norm, ptol * (x_norm + ptol))
                if step_norm <= ptol * (x_norm + ptol):
                    term = PARAMETER_TOLERANCE
                else:
                    near(abs(change), ftol * x_cost)
                    if abs(change) <= ftol * x_cost:
                        term = FUNCTION_TOLERANCE
                    else:
                        rd = change / model
                        near(rd, o["min_relative_decrease"])
                        if rd > num(o["min_relative_decrease"]):
                            X, S, x_cost = Xt, St, cand
                            gmax = max(abs(S[6]), abs(S[7]), abs(S[8]))
                            t = 2 * rd - 1
                            radius = min(num(o["max_radius"]), radius / max(num(1.0) / 3, 1 - t * t * t))
                            factor, last_ok = num(2.0), True
                        else:
                            radius = radius / factor; factor = factor * 2
                            last_ok = False
            if term < 0:
                if last_ok:
                    near(gmax, gtol)
                if it >= o["max_num_iterations"]:
                    term = NO_CONVERGENCE
                elif last_ok and gmax <= gtol:
                    term = GRADIENT_TOLERANCE
                elif radius <= num(o["min_radius"]):
                    term = FAILURE
        if term == FAILURE:
            return out(6, None, num(0.0), it, term, c0, x_cost)
    # ---- step 5 ----
    behind, errs = False, []
    for i in range(n):
        p = tk.project(i, X)
        behind = behind or p[2] < 0
        e = tk.residual(i, p)
        errs.append([e[0] * e[0] + e[1] * e[1]])
    mean = _total(errs, tk.places, tk.length, order, ops)[0] / n
    if not behind:
        near(mean, max_sq)
    status = 4 if behind else 0 if mean < num(max_sq) else 5
    return out(status, X, mean, it, term, c0, x_cost)


def refine_fp64(cams, obs_cam, obs_xy, c, max_sq, loss=HUBER10, options=None, order=None, refine=True):
    with np.errstate(all="ignore"):
        return _refine(cams, obs_cam, obs_xy, c, max_sq, loss, options, order, _Fp64, refine)


def refine_mp(cams, obs_cam, obs_xy, c, max_sq, loss=HUBER10, options=None, refine=True):
    """the point comes back as fp64 (rounded from 50 digits), the costs and the mean as mpf"""
    with mpmath.workdps(tri.MP_DPS):
        return _refine(cams, obs_cam, obs_xy, c, max_sq, loss, options, None, _Mp, refine)


def same_decisions(a, b):
    return (a.status, a.termination, a.iterations) == (b.status, b.termination, b.iterations)


# ----------------------------------------------------- the parity batch ----
HAND_SEED = 9107
HAND_PLACED = ("midpoint_fails_the_gate_refined_passes", "one_outlier_observation", "noise_free", "two_views", "unestimated_in_the_middle",
               "length_8", "length_9", "length_64", "length_65", "length_130")
MAX_FLAGGED_FRACTION = 0.02


def _estimated_in_front(batch, X, min_depth=1.0):
    return [k for k in range(tri.N_CAMS - 1) if batch["estimated"][k]
            and (tri.rotation_matrix(batch["rot_aa"][k]) @ (np.asarray(X) - batch["cam_pos"][k]))[2] > min_depth]


def make_batch():
    """triangulation_reference.make_batch() and, behind it, the tracks of HAND_PLACED; "n_base" is the count of the former"""
    b = tri.make_batch()
    rng = np.random.Generator(np.random.PCG64(HAND_SEED))
    tracks = []

    def seen(cam_list, X, noise):
        return [(c, tri._project(b, c, X) + noise * rng.standard_normal(2)) for c in cam_list]
    # a point close to one camera and far from six: the midpoint weighs every ray's distance alike, so the far cameras' noise lands on the near
    # ones' pixels; the reprojection error of the midpoint is several times that of the refined point
    Q = b["cam_pos"][3] + 1.5 * tri.rotation_matrix(b["rot_aa"][3])[2]           # 1.5 in front of camera 3, on its axis
    front = sorted(_estimated_in_front(b, Q), key=lambda k: np.linalg.norm(b["cam_pos"][k] - Q))
    assert front[0] == 3
    tracks.append(seen(front[:1] + front[-6:], Q, 7.0))
    P = np.array([0.4, -0.3, 0.6])
    cams_p = _estimated_in_front(b, P)
    one = seen(cams_p[:8], P, 0.5)
    one[3] = (one[3][0], one[3][1] + np.array([30.0, 0.0]))
    tracks.append(one)
    tracks.append([(c, np.round(xy * 2.0 ** 30) / 2.0 ** 30) for c, xy in seen(cams_p[8:13], P, 0.0)])      # exact to 2^-30 px
    tracks.append(seen((cams_p[2], cams_p[20]), P, 0.5))
    tracks.append(seen((cams_p[4], tri.UNESTIMATED[0], cams_p[9], cams_p[15], cams_p[22]), P, 0.5))
    for L in (8, 9, 64, 65, 130):
        X = rng.uniform(-1.5, 1.5, 3)
        ok = _estimated_in_front(b, X)
        tracks.append(seen([ok[k % len(ok)] for k in range(L)], X, 0.5))
    assert len(tracks) == len(HAND_PLACED)
    out = dict(b)
    out["n_base"] = len(b["track_ptr"]) - 1
    out["obs_cam"] = np.concatenate([b["obs_cam"], np.array([c for t in tracks for c, _ in t], dtype=np.uint32)])
    out["obs_xy"] = np.vstack([b["obs_xy"], np.array([xy for t in tracks for _, xy in t])])
    out["track_ptr"] = np.concatenate([b["track_ptr"], b["track_ptr"][-1] + np.cumsum([len(t) for t in tracks]).astype(np.uint64)]).astype(np.uint64)
    return out


def hand_index(batch, name):
    return batch["n_base"] + HAND_PLACED.index(name)


# ---------------------------------- the sub-batch of the other losses ----
SUB_SEED = 9108
SUB_PER_CLASS = 8          # per lane class (4, 16, 64): the base tracks with the most and with the fewest iterations under Huber
SUB_HAND_PLACED = ("all_beyond_the_tukey_cut", "one_beyond_the_cut", "at_the_cut", "length_65_mixed")
SUB_LOSSES = {"tukey": TUKEY10, "geman": GEMAN10, "softl1": SOFTL1_10}
SUB_OUTLIER_PLACE = 3      # one_beyond_the_cut: the observation 30 px off
# options at which a refinement runs to its minimiser instead of stopping at a relative cost change of 1e-6: it ends on the gradient, on a step
# of 1e-14 |x|, or at the iteration cap with steps at rounding level
SUB_CONVERGED = {"function_tolerance": 0.0, "parameter_tolerance": 1e-14}
SUB_MIXED_PLACES = (0, 13, 31, 47, 64)     # length_65_mixed: the observations 30 px off, spread over the 64 lanes and the second pass


def _append_tracks(b, tracks):
    out = dict(b)
    out["obs_cam"] = np.concatenate([b["obs_cam"], np.array([c for t in tracks for c, _ in t], dtype=np.uint32)])
    out["obs_xy"] = np.vstack([b["obs_xy"], np.array([xy for t in tracks for _, xy in t])])
    out["track_ptr"] = np.concatenate([b["track_ptr"], b["track_ptr"][-1] + np.cumsum([len(t) for t in tracks]).astype(np.uint64)]).astype(np.uint64)
    return out


def sub_batch_picks(batch, huber_cases):
    """the tracks of the batch that the sub-batch keeps: HAND_PLACED, and per lane class the SUB_PER_CLASS base tracks with the most and the
    fewest iterations in the Huber golden (ties by index; a track that is not refined there -- status 1, 2, 3 -- does not count)"""
    lengths = np.diff(batch["track_ptr"].astype(np.int64))
    picks = [hand_index(batch, k) for k in HAND_PLACED]
    for G in (4, 16, 64):
        of_class = sorted((huber_cases[t]["iterations"], t) for t in range(batch["n_base"])
                          if tri.lane_class(lengths[t]) == G and huber_cases[t]["termination"] >= 0 and not huber_cases[t]["near"])
        assert len(of_class) >= 2 * SUB_PER_CLASS, (G, len(of_class))
        picks += [t for _, t in of_class[:SUB_PER_CLASS]] + [t for _, t in of_class[-SUB_PER_CLASS:]]
    return picks


def make_sub_batch(batch, huber_cases):
    """About sixty tracks for the losses of SUB_LOSSES: sub_batch_picks() of the batch, then the tracks of SUB_HAND_PLACED.  "picks" are the
    indices in the batch, "n_picked" their count."""
    picks = sub_batch_picks(batch, huber_cases)
    ptr = batch["track_ptr"].astype(np.int64)
    rows = np.concatenate([np.arange(ptr[t], ptr[t + 1], dtype=np.int64) for t in picks])
    sub = dict(batch, track_ptr=np.concatenate([[0], np.cumsum(np.diff(ptr)[picks])]).astype(np.uint64), obs_cam=batch["obs_cam"][rows],
               obs_xy=batch["obs_xy"][rows])
    rng = np.random.Generator(np.random.PCG64(SUB_SEED))

    def seen(cam_list, X, noise):
        return [(c, tri._project(batch, c, X) + noise * rng.standard_normal(2)) for c in cam_list]
    P = np.array([0.4, -0.3, 0.6])
    cams_p = _estimated_in_front(batch, P)
    tracks = []
    # every observation 40 px off in one image direction: cameras that look at P from different sides disagree about it, and the midpoint
    # leaves every one of them beyond a cut of 10 px (tests/test_track_refinement_reference.py checks that)
    tracks.append([(c, xy + np.array([40.0, 0.0])) for c, xy in seen(cams_p[:6], P, 0.5)])
    # make_batch()'s outlier construction with EXACT inliers: then the trivial loss without the outlier and Tukey with it (the outlier beyond
    # the cut, the inliers' weights (1 - s / a^2)^2 / 2 equal to 1e-20) have one minimiser, P, and at SUB_CONVERGED's tolerances both runs reach it
    one = seen(cams_p[:8], P, 0.0)
    one[SUB_OUTLIER_PLACE] = (one[SUB_OUTLIER_PLACE][0], one[SUB_OUTLIER_PLACE][1] + np.array([30.0, 0.0]))
    tracks.append(one)
    # one observation whose residual AT THE REFINED POINT (Tukey 10) is 9.95 px: placed by a secant iteration on its offset (the
    # observation weighs next to nothing there, so the refined point hardly follows it)
    at = seen(cams_p[10:18], P, 0.5)
    c, max_sq = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2
    base_xy, k_at = at[2][1].copy(), 2

    def residual_norm(off):
        at[k_at] = (at[k_at][0], base_xy + np.array([off, 0.0]))
        oc, xy = np.array([cc for cc, _ in at], dtype=np.uint32), np.array([v for _, v in at])
        X = refine_fp64(batch, oc, xy, c, max_sq, TUKEY10).point
        return float(np.linalg.norm(tri._project(batch, at[k_at][0], X) - at[k_at][1]))
    o0, o1 = 9.0, 10.0
    f0, f1 = residual_norm(o0) - 9.95, residual_norm(o1) - 9.95
    for _ in range(20):
        if abs(f1) < 1e-3:
            break
        o0, o1, f0 = o1, o1 - f1 * (o1 - o0) / (f1 - f0), f1
        f1 = residual_norm(o1) - 9.95
    assert abs(f1) < 1e-3, f1
    tracks.append(list(at))
    X = rng.uniform(-1.5, 1.5, 3)
    ok = _estimated_in_front(batch, X)
    mixed = seen([ok[k % len(ok)] for k in range(65)], X, 0.5)
    for k in SUB_MIXED_PLACES:
        mixed[k] = (mixed[k][0], mixed[k][1] + np.array([0.0, 30.0]))
    tracks.append(mixed)
    assert len(tracks) == len(SUB_HAND_PLACED)
    out = _append_tracks(sub, tracks)
    out["picks"], out["n_picked"] = picks, len(picks)
    return out


def sub_index(sub, name):
    return sub["n_picked"] + SUB_HAND_PLACED.index(name)


def without_observation(oc, xy, place):
    keep = [k for k in range(len(oc)) if k != place]
    return oc[keep], xy[keep]


def compute_sub_golden(sub):
    """compute_golden() of the sub-batch per loss of SUB_LOSSES, and the 50-digit point of one_beyond_the_cut WITHOUT its outlier under the
    trivial loss and of the track WITH it under Tukey, both at SUB_CONVERGED's tolerances (what Tukey has to reproduce: the observation beyond the
    cut weighs nothing)"""
    doc = {"sub_seed": SUB_SEED, "picks": [int(t) for t in sub["picks"]], "hand_placed": list(SUB_HAND_PLACED),
           "losses": {name: compute_golden(sub, loss) for name, loss in SUB_LOSSES.items()}}
    oc, xy = without_observation(*tri.track_slices(sub)[sub_index(sub, "one_beyond_the_cut")], SUB_OUTLIER_PLACE)
    c, max_sq = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2
    full = tri.track_slices(sub)[sub_index(sub, "one_beyond_the_cut")]
    doc["without_the_outlier"] = {"trivial": [float(x).hex() for x in refine_mp(sub, oc, xy, c, max_sq, TRIVIAL, SUB_CONVERGED).point],
                                  "tukey_with_it": [float(x).hex() for x in refine_mp(sub, *full, c, max_sq, TUKEY10, SUB_CONVERGED).point]}
    return doc


# ------------------------------------------------------ the golden file ----
ORDERS = 8


def relative_cost_deviation(cost, ref_cost):
    return abs(float(cost) - float(ref_cost)) / max(abs(float(ref_cost)), 1e-300)


def compute_golden(batch=None, loss=HUBER10):
    """Per track of the batch: the 50-digit result and the fp64 restatement's worst relative deviation from it (point, as the triangulation
    measures it, and final cost) over ORDERS summation orders -- the given order first, then seeded permutations.  An order whose decisions
    differ from the 50-digit ones (possible on a flagged track only) does not enter the spread."""
    batch = batch or make_batch()
    c, max_sq = tri.cos_min_angle(), tri.MAX_ERR_PX ** 2
    cases = []
    for t, (oc, xy) in enumerate(tri.track_slices(batch)):
        hp = refine_mp(batch, oc, xy, c, max_sq, loss)
        case = {"length": int(len(oc)), "status": hp.status, "n_views": hp.n_views, "point": [float(x).hex() for x in hp.point],
                "mean_sq_err": float(hp.mean_sq_err), "iterations": hp.iterations, "termination": hp.termination,
                "initial_cost": float(hp.initial_cost), "final_cost": float(hp.final_cost), "near": bool(hp.near), "spread": 0.0,
                "fp64_agrees": []}
        rng = np.random.Generator(np.random.PCG64(HAND_SEED + 50000 + t))
        centroid = tri.origin_centroid(batch, oc) if hp.n_views else None
        for k in range(ORDERS if hp.status in (0, 4, 5) else 1):
            lo = refine_fp64(batch, oc, xy, c, max_sq, loss, order=None if k == 0 else rng.permutation(hp.n_views))
            case["fp64_agrees"].append(bool(same_decisions(lo, hp)))
            if hp.status in (0, 4, 5) and same_decisions(lo, hp):
                case["spread"] = max(case["spread"], tri.relative_deviation(lo.point, hp.point, centroid))
                if float(hp.final_cost) > 1e-12:          # below: the cost is the rounding of the pixels, not a quantity to agree on
                    case["spread"] = max(case["spread"], relative_cost_deviation(lo.final_cost, hp.final_cost))
        cases.append(case)
    return {"hand_seed": HAND_SEED, "batch_seed": tri.BATCH_SEED, "orders": ORDERS, "mp_dps": tri.MP_DPS, "loss": json.loads(json.dumps(loss)),
            "min_angle_degrees": tri.MIN_ANGLE_DEG, "max_error_pixels": tri.MAX_ERR_PX, "num_near": sum(cs["near"] for cs in cases),
            "spread_max": max(cs["spread"] for cs in cases), "cases": cases}
