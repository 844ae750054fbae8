"""-m gpu: the bundle adjustment of camera positions and points (include/gsfm_ba.h) against tests/ba_reference.py.

Scenes (ba_reference.scene): (a) 12 cameras / 60 tracks with one unestimated camera and three unestimated tracks; (b) 70 cameras with
tracks of 2, 8, 9, 64, 65 and 70 observations and camera rows of 3, 63, 64, 65 and about 300 observations -- both lane-class boundaries
and the 64-lane row stride.  Bounds: for a quantity Q the device's deviation from the hp tier, max |Q_dev - Q_hp|, is at most
MARGIN x the fp64 tier's own deviation max |Q_fp64 - Q_hp| (ba_reference.MARGIN explains the 64), where the latter is taken as at least
one rounding unit u max |Q_hp| of the quantity: a spread below the precision of the number format is luck, not a bound.  Every test
prints its worst ratio (DESIGN.md section 16 records them).

Scene t is scene b's graph with observations placed beyond a Tukey cut of 10 px at the near start: all three of camera 4 (its B block is
then exactly zero and the Schur complement there is the damping alone), both of the two-view track 5 (C = 0: the min_lm_diagonal clamp
alone, Jacobi scale 1 / (1 + 0)), single ones in long tracks, and two within 1 % of the cut (tests/test_ba_reference.py asserts these
conditions on the reference).  Tukey is the one accepted loss with rho' = 0; Geman-McClure the one that reads a second parameter.
"""
import numpy as np
import pytest

from globalsfmpy_amd import _abi, loss_functions as LF
from globalsfmpy_amd.solver import BundleProblem, SolverError, bundle_adjust_positions_and_points

import ba_reference as R

pytestmark = pytest.mark.gpu

LOSSES = {"trivial": (None, None, None), "huber": (LF.HuberLoss(10.0), "huber", 10.0), "softl1": (LF.SoftLOneLoss(10.0), "softl1", 10.0),
          "tukey": (LF.TukeyLoss(10.0),) + R.TUKEY, "geman": (LF.GemanMcClureLoss(10.0, 0.5),) + R.GEMAN}
CASE_LOSS = {R.LOSS: "huber", R.TUKEY: "tukey", R.GEMAN: "geman"}   # ba_reference.case_loss -> LOSSES
CAM, TRK = R.T_CAMERA, R.T_TRACK


def _problem(sc, loss=None):
    P = BundleProblem(sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"])
    P.set_loss(loss)
    return P


_ratio = R.ratio   # max |dev - hp| / (MARGIN max(max |fp64 - hp|, u max |hp|))


def _report(tag, worst):
    print("%-40s %s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _start(sc):
    return R.perturbed_start(sc, 0.05, 0.05, 1)


# ---- 1. residuals, linearisation, Schur product ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(LOSSES))
@pytest.mark.parametrize("sname", ["a", "b", "t"])
def test_linearisation_and_schur_product_against_hp_reference(sname, lname):
    sc = R.scene(sname)
    loss, kind, a = LOSSES[lname]
    N = len(sc["cam_est"])
    c0, p0 = _start(sc)
    lin64, asm64 = R.point_linearisation(sname, kind, a, False)
    linhp, asmhp = R.point_linearisation(sname, kind, a, True)
    if lname == "huber":   # both branches of the loss occur
        s = lin64["s"][sc["used"]]
        assert (s > 100.0).any() and (s < 100.0).any()
    r64, _ = R.observe_np(sc, c0, p0)
    rhp, _ = R.cached(("obs", sname), lambda: R.observe_hp(sc, c0, p0))
    P = _problem(sc, loss)
    r, rho = P.residuals(c0, p0)
    L = P.linearize(c0, p0)
    worst = {"r": _ratio(r, r64, rhp), "rho": _ratio(rho, lin64["rho"], linhp["rho"]), "cost": _ratio(L["cost"], asm64["cost"], asmhp["cost"]),
             "g_cam": _ratio(L["grad_cam"], asm64["g"][:N], asmhp["g"][:N]), "g_point": _ratio(L["grad_point"], asm64["g"][N:], asmhp["g"][N:]),
             "B": _ratio(L["diag_cam"], asm64["B"], asmhp["B"]), "C": _ratio(L["diag_point"], asm64["C"], asmhp["C"])}
    assert np.all(r[~sc["used"]] == 0) and np.all(rho[~sc["used"]] == 0)
    cut_case = sname == "t" and lname == "tukey"
    if cut_case:   # exact zeros where every observation lies beyond the cut
        tp = sc["track_ptr"].astype(np.int64)
        rows = np.concatenate([np.flatnonzero(sc["obs_cam"] == CAM), np.arange(tp[TRK], tp[TRK + 1])])
        assert np.all(L["diag_cam"][CAM] == 0) and np.all(L["grad_cam"][CAM] == 0)
        assert np.all(L["diag_point"][TRK] == 0) and np.all(L["grad_point"][TRK] == 0)
        assert np.all((r[rows] * r[rows]).sum(1) > 100.0)
        worst["rho_cut"] = _ratio(rho[rows], lin64["rho"][rows], linhp["rho"][rows])   # a^2 / 6 as the hp tier rounds it
    v = np.random.default_rng(3).standard_normal((N, 3))
    for radius in (1e4, 1e10):
        ys = []
        for lin, asm in ((lin64, asm64), (linhp, asmhp)):
            Sc, _, _ = R.schur_system(sc, R.damped(sc, lin, asm, R.jacobi_scale(asm), radius))
            y = (Sc @ v.reshape(-1).astype(Sc.dtype)).reshape(N, 3)
            y[~sc["cam_active"]] = v[~sc["cam_active"]]   # the identity on inactive cameras
            ys.append(y)
        sv = P.schur_matvec(v, radius)
        worst["Sv@%.0e" % radius] = _ratio(sv, ys[0], ys[1])
        if cut_case:   # S reduces to the damping on camera 4's rows
            worst["Sv_cam%d@%.0e" % (CAM, radius)] = _ratio(sv[CAM], ys[0][CAM], ys[1][CAM])
    _report("%s %s" % (sname, lname), worst)


# ---- 2. one LM step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e4, 1e10])
@pytest.mark.parametrize("sname", ["a", "b"])
def test_step_against_refined_hp_solution(sname, radius):
    _step(sname, "huber", radius)


@pytest.mark.parametrize("sname,lname,radius", [("t", "tukey", 1e4), ("t", "tukey", 1e10), ("a", "geman", 1e4)])
def test_step_under_tukey_and_geman_mcclure(sname, lname, radius):
    """Scene t under Tukey: a camera and a point whose blocks are the damping alone; both stay where they are in the plain step.

    [t-tukey-1e10]: beyond the cut scene t also leaves points with ONE observation inside it, a rank-2 block held up by the damping alone
    (1e-10 of its scaled diagonal at this radius).  With every point eliminated by a cofactor inverse in plain fp64 the reduced system
    carried u cond(C~_t), about 1e-6, and was not positive definite as computed; a negative r.M^-1 r was read as a residual of zero and the
    step, 10 493 x its bound off, came back as converged.  Now a breakdown is a stall, and a point whose block is badly conditioned is
    solved in double-double (ba_kernels.hpp: GSFM_BA_DD_COND; every other point keeps its bytes).  On an MI355X: 120 PCG iterations to
    1.4e-14, delta 0.212 of its bound, model cost change 0.016."""
    _step(sname, lname, radius)


def _step(sname, lname, radius):
    sc = R.scene(sname)
    N = len(sc["cam_est"])
    c0, p0 = _start(sc)
    x = np.concatenate([c0, p0])
    loss, kind, a = LOSSES[lname]
    P = _problem(sc, loss)
    st = P.step_check(c0, p0, radius)
    tiers = {}
    for hp in (False, True):
        lin, asm = R.point_linearisation(sname, kind, a, hp)
        y, dm = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), radius, hp=hp)
        delta = R.project_step(sc, dm, y, x.astype(y.dtype))
        model = -(delta * asm["g"]).sum() - R.quad_form(sc, lin, delta) / 2
        tiers[hp] = dict(lin=lin, asm=asm, y=y, dm=dm, delta=delta, model=model, rhs=R.schur_system(sc, dm)[1].reshape(N, 3))
    lo, hi = tiers[False], tiers[True]
    # the reduced system: PCG's true relative residual in the preconditioner norm, against the hp system
    rel, floor = R.pcg_residual_and_floor(sc, hi["dm"], st["y_cam"])
    print("%s radius %.0e: PCG %d iterations, recursion residual %.2e, true residual %.2e, floor %.2e" % (sname, radius, st["cg_iterations"], st["cg_rel"], rel, floor))
    assert not st["stalled"] and st["cg_rel"] <= 1e-12
    assert rel <= 1e-12 + floor
    # back-substitution: the device's points against the hp back-substitution of the device's own camera solution
    yp_hp = R.back_substitute(sc, hi["dm"], np.asarray(st["y_cam"], R.LD).reshape(-1))
    yp_64 = R.back_substitute(sc, lo["dm"], np.asarray(st["y_cam"], np.float64).reshape(-1))
    worst = {"rhs": _ratio(st["rhs"], lo["rhs"], hi["rhs"]), "y_point": _ratio(st["y_point"], yp_64, yp_hp),
             "delta": _ratio(np.concatenate([st["delta_cam"], st["delta_point"]]), lo["delta"], hi["delta"]),
             "model": _ratio(st["model_cost_change"], lo["model"], hi["model"])}
    # the gauge projection: no mean over the active nodes, no component along x - mean(x); inactive nodes do not move
    act = hi["dm"]["act"]
    d = np.concatenate([st["delta_cam"], st["delta_point"]])
    vdir = np.where(act[:, None], x - x[act].mean(0), 0.0)
    dn = np.sqrt((d * d).sum())
    assert np.abs(d[act].mean(0)).max() <= 64 * R.U * dn and abs((d * vdir).sum()) <= 64 * R.U * dn * np.sqrt((vdir * vdir).sum())
    assert np.all(d[~act] == 0)
    # ... and off: Ceres' plain step; J v = 0, so the model cost change is the same
    off = P.step_check(c0, p0, radius, remove_gauge=0)
    assert not off["stalled"]
    if sname == "t" and lname == "tukey":   # zero gradient, zero coupling: y = 0 there (tests/test_ba_reference.py: the reference's is)
        assert np.all(off["delta_cam"][CAM] == 0) and np.all(off["delta_point"][TRK] == 0)
    plain64, plainhp = [R.project_step(sc, t["dm"], t["y"], x.astype(t["y"].dtype), gauge=False) for t in (lo, hi)]
    if radius == 1e4:   # (at 1e10 the plain step's gauge part is set by the damping alone: its conditioning, not the kernels, decides those digits)
        worst["delta_plain"] = _ratio(np.concatenate([off["delta_cam"], off["delta_point"]]), plain64, plainhp)
    models = [-(d_ * t["asm"]["g"]).sum() - R.quad_form(sc, t["lin"], d_) / 2 for d_, t in ((plain64, lo), (plainhp, hi))]
    worst["model_plain"] = _ratio(off["model_cost_change"], models[0], models[1])
    assert abs(float(models[1]) - float(hi["model"])) <= 1e-9 * float(hi["model"])   # (the reference's own: the projection does not change the model)
    _report("%s %s step radius %.0e" % (sname, lname, radius), worst)


# ---- 3. full solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["a0", "b0"])
def test_noise_free_observations_recover_the_generator_scene(sname):
    """Bound: the solve stops at a step of 1e-8 (|x| + 1e-8) or a cost change of 1e-6 of a cost that tends to zero; in normalised
    coordinates (rms 1, |x| <= 20) that leaves an error below 1e-6 (tests/test_ba_reference.py asserts the same of the reference)."""
    sc = R.scene(sname)
    c0, p0 = _start(sc)
    c1, p1, s = _problem(sc).solve(c0, p0)
    err = np.abs(R.normalise(sc, c1, p1) - R.normalise(sc, sc["cam_pos"], sc["gt_points"])).max()
    print(sname, s["termination_name"], s["num_iterations"], "final cost %.3e" % s["final_cost"], "error %.3e" % err)
    assert s["termination"] in (0, 1, 2) and err <= 1e-6


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_noisy_solve_matches_the_reference(name):
    """t_near_tukey: camera 4 and track 5 keep a zero gradient and zero coupling throughout (the reference's stay beyond the cut), so the LM
    step itself never moves them; the default gauge projection does (it subtracts the mean step and the scale component from every active
    node), so they come back with the reference's step, not with their input bytes: bounded with everything else in x, and on their own.

    [a_near_tukey]: scene a under Tukey has two-view tracks with one observation beyond the cut, nearly singular damped blocks from the first
    iteration on.  With plain-fp64 elimination throughout the coordinates ended 1.099 x their bound off the hp tier (counts and costs the
    reference's); with the badly conditioned points solved in double-double they are at 0.785."""
    sc = R.scene(R.CASES[name][0])
    c0, p0 = R.case_start(name)
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    c1, p1, s = _problem(sc, LOSSES[CASE_LOSS[R.case_loss(name)]][0]).solve(c0, p0)
    print(name, s["termination_name"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], "cg", s["num_cg_iterations"],
          "cost %.15e (hp %.15e)" % (s["final_cost"], hi["final_cost"]))
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"]) == \
        (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert s["num_pcg_stalled_steps"] == 0
    if name.endswith("far"):
        assert s["num_unsuccessful_steps"] >= 1
    worst = {"initial_cost": _ratio(s["initial_cost"], lo["initial_cost"], hi["initial_cost"]), "final_cost": _ratio(s["final_cost"], lo["final_cost"], hi["final_cost"]),
             "x": _ratio(R.normalise(sc, c1, p1), R.normalise(sc, lo["cam"], lo["points"]), R.normalise(sc, hi["cam"], hi["points"]))}
    if name == "t_near_tukey":
        nc = int(sc["cam_active"].sum())
        assert sc["cam_active"].all() and sc["pt_active"].all()
        pick = lambda c, p: R.normalise(sc, c, p)[[CAM, nc + TRK]]
        worst["x_cut"] = _ratio(pick(c1, p1), pick(lo["cam"], lo["points"]), pick(hi["cam"], hi["points"]))
        assert not np.array_equal(hi["cam"][CAM], c0[CAM])   # (the reference's camera 4 moves: by the gauge projection alone)
        # ... and without the projection both keep their input bytes (the reference's do: tests/test_ba_reference.py)
        c2, p2, s2 = _problem(sc, LOSSES["tukey"][0]).solve(c0, p0, remove_gauge=0)
        assert s2["termination"] in (0, 1, 2) and s2["num_iterations"] >= 3 and s2["num_pcg_stalled_steps"] == 0
        assert c2[CAM].tobytes() == c0[CAM].tobytes() and p2[TRK].tobytes() == p0[TRK].tobytes()
    _report(name, worst)


# ---- 4. the rest ---------------------------------------------------------------------------------------------------------------
def test_two_solves_return_the_same_bytes_and_inactive_nodes_pass_bit_for_bit():
    sc = R.scene("a")
    c0, p0 = R.case_start("a_near")
    odd = np.array([-0.0, np.nan, 1e300])
    c0[~sc["cam_active"]] = odd
    p0[~sc["pt_active"]] = odd
    assert (~sc["cam_active"]).sum() >= 1 and (~sc["pt_active"]).sum() >= 3
    P = _problem(sc, LOSSES["huber"][0])
    c1, p1, s1 = P.solve(c0, p0)
    c2, p2, s2 = P.solve(c0, p0)
    c3, p3, s3 = bundle_adjust_positions_and_points(sc["rot_aa"], c0, sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], p0, sc["cam_est"],
                                                    sc["pt_est"], loss=LOSSES["huber"][0])
    assert c1.tobytes() == c2.tobytes() == c3.tobytes() and p1.tobytes() == p2.tobytes() == p3.tobytes()
    assert s1["final_cost"] == s2["final_cost"] == s3["final_cost"] and s1["num_cg_iterations"] == s2["num_cg_iterations"]
    assert c1[~sc["cam_active"]].tobytes() == c0[~sc["cam_active"]].tobytes() and p1[~sc["pt_active"]].tobytes() == p0[~sc["pt_active"]].tobytes()
    assert np.all(np.isfinite(c1[sc["cam_active"]])) and not np.array_equal(c1[sc["cam_active"]], c0[sc["cam_active"]])
    assert (s1["num_observations_used"], s1["num_active_cameras"], s1["num_active_points"]) == (sc["used"].sum(), sc["cam_active"].sum(), sc["pt_active"].sum())


def test_a_problem_without_a_used_observation_changes_nothing():
    sc = R.scene("a")
    c0, p0 = R.case_start("a_near")
    P = BundleProblem(sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], np.zeros(12, np.uint8), None)
    c1, p1, s = P.solve(c0, p0)
    assert c1.tobytes() == c0.tobytes() and p1.tobytes() == p0.tobytes() and s["num_observations_used"] == 0 and s["num_iterations"] == 0
    P = BundleProblem(sc["rot_aa"], sc["intrinsics"], np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 2)))
    c1, p1, s = P.solve(c0, np.zeros((0, 3)))
    assert c1.tobytes() == c0.tobytes() and s["num_observations_used"] == 0


def test_argument_and_loss_errors():
    sc = R.scene("a")
    tp = sc["track_ptr"].copy()
    bad_first, bad_order, bad_cam = tp.copy(), tp.copy(), sc["obs_cam"].copy()
    bad_first[0] = 1
    bad_order[5] = bad_order[4] - 1
    bad_cam[7] = 12
    for kw in (dict(track_ptr=bad_first), dict(track_ptr=bad_order), dict(obs_cam=bad_cam)):
        a = dict(track_ptr=tp, obs_cam=sc["obs_cam"])
        a.update(kw)
        with pytest.raises(SolverError, match="status 1"):
            BundleProblem(sc["rot_aa"], sc["intrinsics"], a["track_ptr"], a["obs_cam"], sc["obs_xy"])
    P = _problem(sc)
    for nodes in ([(_abi.LOSS_MAGSAC, 0.02, 9.0, 0.0)], [(1, 10.0, 0, 0), (1, 10.0, 0, 0)], [(1, -1.0, 0, 0)],
                  [(3, 10.0, 0, 0)]):
        with pytest.raises(SolverError, match="status 1"):
            P.set_loss(nodes)
    # every leaf loss_leaf_simple does not evaluate is refused (it would run as no loss at all); Tukey and Geman-McClure are taken
    for kind in (_abi.LOSS_CAUCHY, _abi.LOSS_ARCTAN, _abi.LOSS_TOLERANT, _abi.LOSS_LONE_HALF, _abi.LOSS_LTWO, _abi.LOSS_MAGSAC, _abi.LOSS_MAGSAC + 1, 99):
        with pytest.raises(SolverError, match="status 1"):
            P.set_loss([(kind, 10.0, 0.5, 0.0)])
    for nodes in ([(_abi.LOSS_TUKEY, 0.0, 0, 0)], [(_abi.LOSS_TUKEY, float("nan"), 0, 0)], [(_abi.LOSS_GEMAN_MCCLURE, -1.0, 0.5, 0)], [(_abi.LOSS_GEMAN_MCCLURE, 10.0, float("inf"), 0)]):
        with pytest.raises(SolverError, match="status 1"):
            P.set_loss(nodes)
    P.set_loss([(_abi.LOSS_TUKEY, 10.0, 0, 0)])
    P.set_loss([(_abi.LOSS_GEMAN_MCCLURE, 10.0, 0.5, 0)])
    P.set_loss(LF.TukeyLoss(10.0))
    P.set_loss(LF.GemanMcClureLoss(10.0, 0.5))
    with pytest.raises(SolverError, match="status 1"):
        P.schur_matvec(np.zeros((12, 3)))   # no linearisation yet
    with pytest.raises(SolverError, match="status 1"):
        P.step_check(sc["cam_pos"], sc["gt_points"], radius=0.0)
