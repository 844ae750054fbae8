"""-m gpu: position estimation with point-to-camera constraints (include/gsfm_posp.h) against tests/position_points_reference.py (float64)
and tests/position_points_hp_reference.py (mpmath / long double).

The scene (position_points_reference.make_scene): 72 cameras, 300 edges, 91 tracks with CSR lengths on both sides of the lane classes'
limits, a camera row that wraps the wavefront, the fixed camera observed by several tracks, a track with one used observation (inactive),
two cameras without an edge, a camera with edges and no observation; the evaluation point (perturbed_start) puts two cameras on one centre
and a point on its camera, so the guard is taken on the edge and on the observation side.

Bounds.  Check 1 is componentwise in the style of tests/test_gpu_positions_hp.py, with its constants C0 = 64 (roundings per summand) and
CA = 16 (rows), on the error scales of position_hp_reference extended by w_p (e_mag = 2 w_p, Jw = 2 w_p / n for an observation).  The ray has
no like there: its error scale is |ray| = 1 per component, and C_RAY is the next power of two at or above 4 x the worst ratio measured on an
MI355X (DESIGN.md section 21 records the measurement).  Checks 2 and 3 use tests/test_gpu_ba.py's bound: the device's deviation from the hp
tier is at most ba_reference.MARGIN x the float64 tier's own, taken as at least one rounding unit of the quantity.
"""
import numpy as np
import pytest

from globalsfmpy_amd import _abi, loss_functions as LF
from globalsfmpy_amd.solver import PointPositionProblem, PositionProblem, SolverError, estimate_positions_with_points

import ba_reference as BR
import hp_reference as H
import position_hp_reference as PH
import position_points_hp_reference as PPH
import position_points_reference as PR

pytestmark = pytest.mark.gpu

U, LD = H.U, H.LD
C0, CA, ALLOW_MEDIAN = 64.0, 16.0, 1e-11   # tests/test_gpu_positions_hp.py's
C_RAY = 8.0                                # measured worst ratio 1.705 (u per component): 4 x 1.705 = 6.8 -> 8
W_P = 0.37
LOSSES = {"trivial": (None, None, ()), "huber": (LF.HuberLoss(0.1), "huber", (0.1,)), "cauchy": (LF.CauchyLoss(0.1), "cauchy", (0.1,)),
          "tolerant": (LF.TolerantLoss(0.05, 0.1), "tolerant", (0.05, 0.1))}   # cauchy and tolerant run as LM_PROGRAM; tolerant has rho'' > 0
_ratio = BR.ratio
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _problem(sc, loss=None, weight=W_P, tracks=True):
    kw = dict(ray_rot_aa=sc["ray_rot_aa"], intrinsics=sc["intrinsics"], track_ptr=sc["track_ptr"], obs_cam=sc["obs_cam"], obs_xy=sc["obs_xy"]) if tracks else {}
    P = PointPositionProblem(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], point_to_camera_weight=weight, **kw)
    P.set_loss(loss)
    return P


def _reference(sc, loss=None, weight=W_P):
    return PR.PointPositionReference(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], sc["ray_rot_aa"], sc["intrinsics"],
                                     sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], weight, loss)


def _eval_scene():
    sc = PR.make_scene(noise=0.01, outlier_frac=0.1)
    c0, p0 = PR.perturbed_start(sc, 0.3, 1)
    return sc, c0, p0


def _tier1():
    sc, c0, p0 = _eval_scene()
    return cached("tier1", lambda: PPH.joint_edge_set(sc, c0, p0, W_P))


def _report(tag, worst, allow=None):
    print("%-32s %s%s" % (tag, "  ".join("%s %.3g" % kv for kv in worst.items()),
                          "" if not allow else " | allowed rel. median " + " ".join("%s %.1e" % kv for kv in allow.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    loose = {k: a for k, a in (allow or {}).items() if not a <= ALLOW_MEDIAN}
    assert not loose, ("vacuous bound", tag, loose)


# ---- 1. rays, residuals, rho, cost, gradients, diagonal blocks ----------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(LOSSES))
def test_linearisation_against_hp_reference(lname):
    sc, c0, p0 = _eval_scene()
    loss, kind, params = LOSSES[lname]
    ref = _tier1()
    lin = PH.corrected(ref, kind, params)
    N, E, nn, ei, ej, used = sc["n_cams"], ref["n_edges"], ref["n_nodes"], ref["ei"], ref["ej"], ref["used"]
    assert (~ref["unit"][:E]).sum() == 1 and (~ref["unit"][E:]).sum() == 1   # the guard on either side
    if lname == "huber":
        s = lin["s"].astype(float)
        assert (s > 0.01).any() and (s < 0.01).any() and np.all(np.abs(s - 0.01) > 1e-11)
    if lname == "tolerant":
        assert (lin["rho"][2][:E] > 0).sum() > E // 4 and (lin["rho"][2][E:] > 0).sum() > (len(ei) - E) // 4   # the Corrector's alpha branch
    P = _problem(sc, loss)
    res = P.residuals(c0, p0)
    worst = {"ray": H.ratio(res["ray"], ref["ray"], C_RAY * U * np.ones(3))}
    print("ray: worst |dev - hp| / u = %.3f (C_RAY %g)" % (float(np.abs(res["ray"].astype(LD) - ref["ray"]).max()) / U, C_RAY))
    assert np.all(res["ray"][~used] == 0) and np.all(res["r_obs"][~used] == 0) and np.all(res["rho_obs"][~used] == 0) and (~used).sum() >= 3
    r_dev = np.concatenate([res["r_edge"], res["r_obs"][used]])
    rho_dev = np.concatenate([res["rho_edge"], res["rho_obs"][used]])
    emag = ref["e_mag"]
    worst["r"] = H.ratio(r_dev, ref["r"], C0 * U * emag)
    sb = C0 * U * (lin["s"] + 2 * (np.abs(ref["r"]) * emag).sum(axis=1)) + ((C0 * U * emag) ** 2).sum(axis=1)
    rho0, rho1, rho2 = lin["rho"]
    worst["rho"] = H.ratio(rho_dev, rho0, C0 * U * lin["rho_scale"] + rho1 * sb)
    L = P.linearize(c0, p0)
    worst["cost"] = H.ratio(L["cost"], LD(0.5) * rho0.sum(), 0.5 * ((C0 + len(ei)) * U * lin["rho_scale"] + rho1 * sb).sum())
    A = H.assemble(lin, nn, ei, ej)
    ck = H.c_row(A["deg"], CA)
    g_dev = np.concatenate([L["grad_cam"], L["grad_point"]])
    D_dev = np.concatenate([L["diag_cam"], L["diag_point"]])
    bounds = {"g": (ck[:, None] * U * A["g_mag"], A["g_true"]), "D": (ck[:, None, None] * U * A["D_mag"], A["D_true"])}
    worst["g_cam"] = H.ratio(g_dev[:N], A["g"][:N], bounds["g"][0][:N])
    worst["g_point"] = H.ratio(g_dev[N:], A["g"][N:], bounds["g"][0][N:])
    worst["diag_cam"] = H.ratio(D_dev[:N], A["D"][:N], bounds["D"][0][:N])
    worst["diag_point"] = H.ratio(D_dev[N:], A["D"][N:], bounds["D"][0][N:])
    idle = np.r_[list(PR.EDGELESS), N + PR.SINGLE_TRACK]
    assert np.all(g_dev[idle] == 0) and np.all(D_dev[idle] == 0) and A["deg"][idle].sum() == 0
    assert A["deg"][PR.HUB] > 64 + 2 and A["deg"][PR.NO_OBS_CAM] == np.sum(sc["edge_i"] == PR.NO_OBS_CAM) + np.sum(sc["edge_j"] == PR.NO_OBS_CAM)
    P.close()
    _report("linearisation " + lname, worst, {k: H.allowed_relative(b, t) for k, (b, t) in bounds.items()})


# ---- 2, 3. the reduced operator and one LM step ----------------------------------------------------------------------------------------
def _tiers(lname, radius):
    """{False: float64 tier, True: long-double tier}: the damped system of the full problem, its Schur complement, the step"""
    def make():
        sc, c0, p0 = _eval_scene()
        loss, kind, params = LOSSES[lname]
        ref = _tier1()
        N, nn = sc["n_cams"], ref["n_nodes"]
        st = ref["structure"]
        act = np.concatenate([st["present"], st["point_active"]])
        act[sc["fixed"]] = False
        out = {}
        for hp in (False, True):
            if hp:
                lin = PH.corrected(ref, kind, params)
                Lm, g = PPH.normal_system(lin["Jjt"], lin["rt"], ref["ei"], ref["ej"], nn, LD)
            else:
                r64 = _reference(sc, loss)
                _, _, A, rt, _ = r64.linearize(r64.joint(c0, p0))
                assert np.array_equal(r64.ei, ref["ei"]) and np.array_equal(r64.ej, ref["ej"])
                Lm, g = PPH.normal_system(A, rt, r64.ei, r64.ej, nn, np.float64)
            sysm = PPH.damped_system(Lm, g, act, radius, LD if hp else np.float64)
            Sc, rhs, Mb = PPH.schur_system(sysm, N)
            y = PPH.solve_full(sysm)
            x = np.concatenate([c0, p0])
            delta, model = PPH.project_step(sysm, y, x, sc["fixed"])
            plain, model_plain = PPH.project_step(sysm, y, x, sc["fixed"], gauge=False)
            out[hp] = dict(sys=sysm, Sc=Sc, rhs=rhs, Mb=Mb, y=y, delta=delta, model=model, plain=plain, model_plain=model_plain, act=act)
        return out
    return cached(("tiers", lname, radius), make)


@pytest.mark.parametrize("lname", ["huber", "tolerant"])
def test_schur_product_against_explicit_schur_complement(lname):
    sc, c0, p0 = _eval_scene()
    N = sc["n_cams"]
    P = _problem(sc, LOSSES[lname][0])
    P.step_check(c0, p0, fixed_cam=sc["fixed"], max_cg_iterations=1)   # the linearisation and the active set (the fixed camera inactive)
    rng = np.random.default_rng(3)
    worst = {}
    for radius in (1e4, 1e10):
        t = _tiers(lname, radius)
        cam_act = t[True]["act"][:N]
        assert (~cam_act).sum() == 3
        for name, v in (("unit", np.eye(3)[np.arange(N) % 3]), ("rand", rng.standard_normal((N, 3)))):
            ys = [(t[hp]["Sc"] @ v.reshape(-1).astype(t[hp]["Sc"].dtype)).reshape(N, 3) for hp in (False, True)]
            sv = P.schur_matvec(v, radius)
            assert np.array_equal(sv[~cam_act], v[~cam_act])   # the identity on inactive cameras
            worst["Sv_%s@%.0e" % (name, radius)] = _ratio(sv, ys[0], ys[1])
    P.close()
    _report("schur product " + lname, worst)


def _minv_norm(Mb, vec):
    v = np.asarray(vec, LD).reshape(-1, 3)
    return np.sqrt(np.einsum("ka,kab,kb->", v, H.sym3_inverse(np.asarray(Mb, LD)), v))


@pytest.mark.parametrize("radius", [1e4, 1e10])
@pytest.mark.parametrize("lname", ["huber", "tolerant"])
def test_step_against_hp_step_from_the_full_system(lname, radius):
    sc, c0, p0 = _eval_scene()
    N = sc["n_cams"]
    x = np.concatenate([c0, p0])
    P = _problem(sc, LOSSES[lname][0])
    st = P.step_check(c0, p0, fixed_cam=sc["fixed"], radius=radius)
    t = _tiers(lname, radius)
    lo, hi = t[False], t[True]
    # the reduced system: PCG's true relative residual in the preconditioner norm against the hp system, and its attainable-accuracy floor
    y = np.asarray(st["y_cam"], LD).reshape(-1)
    nb = _minv_norm(hi["Mb"], hi["rhs"])
    rel = float(_minv_norm(hi["Mb"], hi["rhs"] - hi["Sc"] @ y) / nb)
    K, c = hi["sys"]["K"], 3 * N
    Cabs = np.abs(np.linalg.inv(np.array(K[c:, c:], float))).astype(LD)   # (block diagonal)
    Sa = np.abs(K[:c, :c]) + np.abs(K[:c, c:]) @ Cabs @ np.abs(K[c:, :c])
    ra = np.abs(hi["sys"]["b"][:c]) + np.abs(K[:c, c:]) @ Cabs @ np.abs(hi["sys"]["b"][c:])
    floor = float(BR.MARGIN * U * _minv_norm(hi["Mb"], Sa @ np.abs(y) + ra) / nb)
    print("%s radius %.0e: PCG %d iterations, recursion residual %.2e, true residual %.2e, floor %.2e" % (lname, radius, st["cg_iterations"], st["cg_rel"], rel, floor))
    assert not st["stalled"] and st["cg_rel"] <= 1e-12
    assert rel <= 1e-12 + floor
    yp_hp = PPH.back_substitute(hi["sys"], N, np.asarray(st["y_cam"], LD))
    yp_64 = PPH.back_substitute(lo["sys"], N, np.asarray(st["y_cam"], np.float64))
    d = np.concatenate([st["delta_cam"], st["delta_point"]]).reshape(-1)
    worst = {"rhs": _ratio(st["rhs"].reshape(-1), lo["rhs"], hi["rhs"]), "y_point": _ratio(st["y_point"], yp_64, yp_hp),
             "delta": _ratio(d, lo["delta"], hi["delta"]), "model": _ratio(st["model_cost_change"], lo["model"], hi["model"])}
    # the gauge projection: no component along x - x_fixed over the active nodes; inactive nodes do not move
    act = hi["act"]
    vdir = np.where(act[:, None], x - x[sc["fixed"]], 0.0).reshape(-1)
    dn = np.sqrt((d * d).sum())
    assert abs((d * vdir).sum()) <= 64 * U * dn * np.sqrt((vdir * vdir).sum())
    assert np.all(d.reshape(-1, 3)[~act] == 0) and (~act).sum() == 4
    off = P.step_check(c0, p0, fixed_cam=sc["fixed"], radius=radius, remove_scale_gauge=0)
    assert not off["stalled"]
    if radius == 1e4:   # (at 1e10 the plain step's gauge part is set by the damping alone: its conditioning, not the kernels, decides those digits)
        worst["delta_plain"] = _ratio(np.concatenate([off["delta_cam"], off["delta_point"]]).reshape(-1), lo["plain"], hi["plain"])
    worst["model_plain"] = _ratio(off["model_cost_change"], lo["model_plain"], hi["model_plain"])
    assert abs(float(hi["model_plain"]) - float(hi["model"])) <= 1e-9 * float(hi["model"])   # (J v = 0: the projection does not change the model)
    # the first PCG iterate, row by row: alpha M^-1 rhs with the hp preconditioner blocks
    one = P.step_check(c0, p0, fixed_cam=sc["fixed"], radius=radius, max_cg_iterations=1)
    y1 = [PPH.first_pcg_iterate(t[hp]["Sc"], t[hp]["rhs"], t[hp]["Mb"]).reshape(N, 3) for hp in (False, True)]
    assert one["cg_iterations"] == 1
    worst["first_iterate_rows"] = max(_ratio(one["y_cam"][k], y1[0][k], y1[1][k]) if np.abs(y1[1][k]).max() > 0 else float(np.abs(one["y_cam"][k]).max() > 0)
                                      for k in range(N))
    worst["first_iterate"] = _ratio(one["y_cam"], y1[0], y1[1])
    P.close()
    _report("step %s radius %.0e" % (lname, radius), worst)


# ---- 4. solves ---------------------------------------------------------------------------------------------------------------------
def _gauge_err(sc, st, ca, pa, cb, pb):
    return float(np.abs(PR.gauge_normalize(ca, pa, sc["fixed"], st["present"], st["point_active"])
                        - PR.gauge_normalize(cb, pb, sc["fixed"], st["present"], st["point_active"])).max())


def test_noise_free_scene_recovers_the_ground_truth():
    sc = PR.make_scene()
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    c, p, s = _problem(sc, None, weight=0.5).solve(fixed_cam=sc["fixed"])
    err = _gauge_err(sc, st, c, p, sc["gt_pos"], sc["gt_points"])
    print("noise-free:", s["termination_name"], s["num_iterations"], "cg", s["num_cg_iterations"], "final cost %.3e" % s["final_cost"], "gauge error %.3e" % err)
    assert s["nonfinite"] == 0 and s["termination"] != 4 and s["num_pcg_stalled_steps"] == 0 and s["num_dense_solves"] == 0
    assert np.all(c[sc["fixed"]] == 0.0)
    assert err <= 1e-8
    assert (s["num_edges_used"], s["num_observations_used"], s["num_active_points"]) == (len(sc["edge_i"]), st["used"].sum(), st["point_active"].sum())


NOISY = dict(noise=0.01, outlier_frac=0.1, seed=5)   # tests/test_position_points_reference.py: the reference's count is stable on this seed


def test_noisy_solve_matches_the_reference():
    sc = PR.make_scene(**NOISY)
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    loss = LF.HuberLoss(0.1)
    cd, pd, sd = _problem(sc, loss, weight=0.5).solve(fixed_cam=sc["fixed"])
    cr, pr, sr = _reference(sc, loss, weight=0.5).solve_joint(fixed_cam=sc["fixed"])
    err = _gauge_err(sc, st, cd, pd, cr, pr)
    print("noisy:", sd["termination_name"], sd["num_iterations"], "reference", sr["termination"], sr["num_iterations"], "cost %.15e (reference %.15e)"
          % (sd["final_cost"], sr["final_cost"]), "gauge error %.3e" % err, "cg", sd["num_cg_iterations"])
    assert (sd["termination"], sd["num_iterations"]) == (sr["termination"], sr["num_iterations"])
    assert sd["final_cost"] == pytest.approx(sr["final_cost"], rel=1e-9, abs=1e-300)
    assert err <= 1e-6


# ---- 5. limits -----------------------------------------------------------------------------------------------------------------------
def test_without_tracks_the_problem_is_the_position_problem():
    sc, c0, _ = _eval_scene()
    loss = LF.HuberLoss(0.1)
    A = PositionProblem(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"])
    A.set_loss(loss)
    B = _problem(sc, loss, tracks=False)
    la, lb = A.linearize(c0), B.linearize(c0, None)
    assert np.float64(la["cost"]).tobytes() == np.float64(lb["cost"]).tobytes()
    assert la["gradient"].tobytes() == lb["grad_cam"].tobytes() and la["diag_blocks"].tobytes() == lb["diag_cam"].tobytes()
    xa, sa = A.solve(None, fixed_cam=sc["fixed"], dense_max_cams=0)
    xb, _, sb = B.solve(fixed_cam=sc["fixed"])
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    none = np.zeros((0, 3))
    err = _gauge_err(sc, st, xa, none, xb, none)
    print("no tracks: iterations %d / %d, gauge error %.3e" % (sa["num_iterations"], sb["num_iterations"], err))
    assert sa["num_iterations"] == sb["num_iterations"] and sa["termination"] == sb["termination"] and err <= 1e-9
    assert sb["num_observations_used"] == 0 and sb["num_active_points"] == 0
    A.close(); B.close()


def test_a_vanishing_weight_leaves_the_camera_only_solve():
    """Noisy edges and observations without outlier edges, HUBER 0.1: the camera-only minimum is isolated, and with w_p = 1e-12 the points add
    1e-24 of the cost, so the cameras end within 1e-6 of the camera-only solve (the float64 reference's two solves: 2.8e-8), while
    w_p = 0.5 moves them by 5.8e-3.  The scene with 10 % outlier edges is not used here: there the two solves, which walk different
    trust-region paths (x and the step carry the points), stop on the function tolerance at different iterations (23 and 29), and the
    float64 reference's own two results lie 1.3e-2 apart (2.4e-4 with both tolerances at 1e-12): a property of that cost surface under
    Ceres' stopping rules, not of the kernels -- the device returned the reference's 1.258e-2 to three digits."""
    sc = PR.make_scene(noise=0.01, outlier_frac=0.0)
    loss = LF.HuberLoss(0.1)
    A = PositionProblem(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"])
    A.set_loss(loss)
    xa, sa = A.solve(None, fixed_cam=sc["fixed"], dense_max_cams=0)
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    errs = {}
    for w in (1e-12, 0.5):
        xb, _, sb = _problem(sc, loss, weight=w).solve(fixed_cam=sc["fixed"])
        errs[w] = _gauge_err(sc, st, xa, np.zeros((0, 3)), xb, np.zeros((0, 3)))
        print("w_p = %g: gauge error of the cameras against the camera-only solve %.3e (%d / %d iterations)" % (w, errs[w], sa["num_iterations"], sb["num_iterations"]))
    assert errs[1e-12] <= 1e-6
    assert errs[0.5] >= 1e-4   # (the limit is not vacuous: a weight of Theia's size moves the cameras)


def test_two_solves_return_the_same_bytes_and_inactive_nodes_pass_bit_for_bit():
    sc = PR.make_scene(**NOISY)
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    c0, p0 = PR.perturbed_start(sc, 0.3, 2)
    odd = np.array([-0.0, np.nan, 1e300])
    c0[list(PR.EDGELESS)] = odd
    p0[~st["point_active"]] = odd
    loss = LF.HuberLoss(0.1)
    P = _problem(sc, loss)
    c1, p1, s1 = P.solve(c0, p0, fixed_cam=sc["fixed"])
    c2, p2, s2 = P.solve(c0, p0, fixed_cam=sc["fixed"])
    c3, p3, s3 = estimate_positions_with_points(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"],
                                                sc["obs_xy"], W_P, cam_pos=c0, points=p0, fixed_cam=sc["fixed"], loss=loss)
    assert c1.tobytes() == c2.tobytes() == c3.tobytes() and p1.tobytes() == p2.tobytes() == p3.tobytes()
    assert s1["final_cost"] == s2["final_cost"] == s3["final_cost"] and s1["num_cg_iterations"] == s2["num_cg_iterations"]
    idle = list(PR.EDGELESS) + [sc["fixed"]]
    assert c1[idle].tobytes() == c0[idle].tobytes() and p1[~st["point_active"]].tobytes() == p0[~st["point_active"]].tobytes()
    assert (~st["point_active"]).sum() == 1 and s1["termination"] != 4 and s1["num_iterations"] >= 2
    moved = np.ones(sc["n_cams"], bool)
    moved[idle] = False
    assert np.all(np.isfinite(c1[moved])) and np.all(np.isfinite(p1[st["point_active"]])) and not np.array_equal(c1[moved], c0[moved])


class PyHuber(object):
    """a loss without a native program: the host-callback path, which this problem refuses"""

    def Evaluate(self, s, out):
        LF.HuberLoss(0.1).Evaluate(s, out)


def test_callback_loss_and_bad_arguments_are_refused():
    sc = PR.make_scene()
    P = _problem(sc)
    with pytest.raises(SolverError, match="status 1"):
        P.set_loss(PyHuber())
    with pytest.raises(SolverError, match="status 1"):
        P.schur_matvec(np.zeros((72, 3)))   # no linearisation yet
    with pytest.raises(SolverError, match="status 1"):
        P.step_check(sc["gt_pos"], sc["gt_points"], radius=0.0)
    for fixed in (PR.EDGELESS[0], 72, -2):
        with pytest.raises(SolverError, match="status 1"):
            P.solve(fixed_cam=fixed)
    P.close()
    tp, oc, ei = sc["track_ptr"].copy(), sc["obs_cam"].copy(), sc["edge_i"].copy()
    bad_first, bad_order, bad_cam, bad_edge = tp.copy(), tp.copy(), oc.copy(), ei.copy()
    bad_first[0] = 1
    bad_order[5] = bad_order[4] - 1
    bad_cam[7] = 72
    bad_edge[3] = 72
    for kw in (dict(track_ptr=bad_first), dict(track_ptr=bad_order), dict(obs_cam=bad_cam), dict(edge_i=bad_edge), dict(weight=0.0), dict(weight=-1.0),
               dict(weight=float("nan")), dict(weight=float("inf"))):
        a = dict(track_ptr=tp, obs_cam=oc, edge_i=ei, weight=0.5)
        a.update(kw)
        with pytest.raises(SolverError, match="status 1"):
            PointPositionProblem(72, a["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], sc["ray_rot_aa"], sc["intrinsics"], a["track_ptr"], a["obs_cam"],
                                 sc["obs_xy"], a["weight"])
    lib = _abi.load_library()
    assert lib.gsfm_posp_set_loss_callback(None, _abi.LOSS_CALLBACK_FN(), None) == 1   # refused before the handle is read
