"""-m gpu: the bundle adjustment of camera positions and points (include/gsfm_ba.h) against tests/ba_reference.py.

Scenes (ba_reference.scene): (a) 12 cameras / 60 tracks with one unestimated camera and three unestimated tracks; (b) 70 cameras with
tracks of 2, 8, 9, 64, 65 and 70 observations and camera rows of 3, 63, 64, 65 and about 300 observations -- both lane-class boundaries
and the 64-lane row stride.  Bounds: for a quantity Q the device's deviation from the hp tier, max |Q_dev - Q_hp|, is at most
MARGIN x the fp64 tier's own deviation max |Q_fp64 - Q_hp| (ba_reference.MARGIN explains the 64), where the latter is taken as at least
one rounding unit u max |Q_hp| of the quantity: a spread below the precision of the number format is luck, not a bound.  Every test
prints its worst ratio (DESIGN.md section 16 records them).
"""
import numpy as np
import pytest

from globalsfmpy_amd import _abi, loss_functions as LF
from globalsfmpy_amd.solver import BundleProblem, SolverError, bundle_adjust_positions_and_points

import ba_reference as R

pytestmark = pytest.mark.gpu

LOSSES = {"trivial": (None, None, None), "huber": (LF.HuberLoss(10.0), "huber", 10.0), "softl1": (LF.SoftLOneLoss(10.0), "softl1", 10.0)}


def _problem(sc, loss=None):
    P = BundleProblem(sc["rot_aa"], sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"])
    P.set_loss(loss)
    return P


def _ratio(dev, fp64, hp):
    """max |dev - hp| / (MARGIN max(max |fp64 - hp|, u max |hp|))"""
    hp = np.asarray(hp, R.LD)
    e_dev = float(np.abs(np.asarray(dev, R.LD) - hp).max())
    e_ref = float(np.abs(np.asarray(fp64, R.LD) - hp).max())
    return e_dev / (R.MARGIN * max(e_ref, R.U * float(np.abs(hp).max())))


def _report(tag, worst):
    print("%-40s %s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _start(sc):
    return R.perturbed_start(sc, 0.05, 0.05, 1)


# ---- 1. residuals, linearisation, Schur product ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(LOSSES))
@pytest.mark.parametrize("sname", ["a", "b"])
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
    v = np.random.default_rng(3).standard_normal((N, 3))
    for radius in (1e4, 1e10):
        ys = []
        for lin, asm in ((lin64, asm64), (linhp, asmhp)):
            Sc, _, _ = R.schur_system(sc, R.damped(sc, lin, asm, R.jacobi_scale(asm), radius))
            y = (Sc @ v.reshape(-1).astype(Sc.dtype)).reshape(N, 3)
            y[~sc["cam_active"]] = v[~sc["cam_active"]]   # the identity on inactive cameras
            ys.append(y)
        worst["Sv@%.0e" % radius] = _ratio(P.schur_matvec(v, radius), ys[0], ys[1])
    _report("%s %s" % (sname, lname), worst)


# ---- 2. one LM step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e4, 1e10])
@pytest.mark.parametrize("sname", ["a", "b"])
def test_step_against_refined_hp_solution(sname, radius):
    sc = R.scene(sname)
    N = len(sc["cam_est"])
    c0, p0 = _start(sc)
    x = np.concatenate([c0, p0])
    P = _problem(sc, LOSSES["huber"][0])
    st = P.step_check(c0, p0, radius)
    tiers = {}
    for hp in (False, True):
        lin, asm = R.point_linearisation(sname, "huber", 10.0, hp)
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
    plain64, plainhp = [R.project_step(sc, t["dm"], t["y"], x.astype(t["y"].dtype), gauge=False) for t in (lo, hi)]
    if radius == 1e4:   # (at 1e10 the plain step's gauge part is set by the damping alone: its conditioning, not the kernels, decides those digits)
        worst["delta_plain"] = _ratio(np.concatenate([off["delta_cam"], off["delta_point"]]), plain64, plainhp)
    models = [-(d_ * t["asm"]["g"]).sum() - R.quad_form(sc, t["lin"], d_) / 2 for d_, t in ((plain64, lo), (plainhp, hi))]
    worst["model_plain"] = _ratio(off["model_cost_change"], models[0], models[1])
    assert abs(float(models[1]) - float(hi["model"])) <= 1e-9 * float(hi["model"])   # (the reference's own: the projection does not change the model)
    _report("%s step radius %.0e" % (sname, radius), worst)


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
    sc = R.scene(R.CASES[name][0])
    c0, p0 = R.case_start(name)
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    c1, p1, s = _problem(sc, LOSSES["huber"][0]).solve(c0, p0)
    print(name, s["termination_name"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], "cg", s["num_cg_iterations"],
          "cost %.15e (hp %.15e)" % (s["final_cost"], hi["final_cost"]))
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"]) == \
        (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert s["num_pcg_stalled_steps"] == 0
    if name.endswith("far"):
        assert s["num_unsuccessful_steps"] >= 1
    worst = {"initial_cost": _ratio(s["initial_cost"], lo["initial_cost"], hi["initial_cost"]), "final_cost": _ratio(s["final_cost"], lo["final_cost"], hi["final_cost"]),
             "x": _ratio(R.normalise(sc, c1, p1), R.normalise(sc, lo["cam"], lo["points"]), R.normalise(sc, hi["cam"], hi["points"]))}
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
    with pytest.raises(SolverError, match="status 1"):
        P.schur_matvec(np.zeros((12, 3)))   # no linearisation yet
    with pytest.raises(SolverError, match="status 1"):
        P.step_check(sc["cam_pos"], sc["gt_points"], radius=0.0)
