"""-m gpu: the full bundle adjustment with free focal lengths (include/gsfm_ba7.h) against tests/ba7_reference.py.

Scenes, losses and bounds are test_gpu_ba6.py's: for a quantity Q the device's deviation from the hp tier is at most MARGIN x the fp64 tier's
own deviation from the hp tier, the latter taken as at least one rounding unit u max |Q_hp| of the quantity.  Every test prints its worst
ratio (DESIGN.md section 19 records them).  Every start perturbs the focal lengths as well.

Scene t (ba_reference.scene_t placed at ba7_reference's near start) puts all of camera 4's observations and both of track 5's beyond a Tukey
cut of 10 px: a 7 x 7 camera block that is the damping alone, and points left with one observation inside the cut, for which the plain-fp64
preconditioner block comes out indefinite at radius 1e10 (k_fba_cam_precond sums such a row again, at either camera dimension).
"""
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi, loss_functions as LF
from globalsfmpy_amd.solver import FocalBundleProblem, SolverError, bundle_adjust_focal

import ba_reference as B
import ba6_reference as R6
import ba7_reference as R

pytestmark = pytest.mark.gpu

LOSSES = {"trivial": (None, None, None), "huber": (LF.HuberLoss(10.0), "huber", 10.0), "softl1": (LF.SoftLOneLoss(10.0), "softl1", 10.0),
          "tukey": (LF.TukeyLoss(10.0),) + B.TUKEY, "geman": (LF.GemanMcClureLoss(10.0, 0.5),) + B.GEMAN}
CASE_LOSS = {B.LOSS: "huber", B.TUKEY: "tukey", B.GEMAN: "geman"}
CAM, TRK = B.T_CAMERA, B.T_TRACK
MIXED = np.arange(12) % 3 != 1   # scene a: the focal lengths of cameras 1, 4, 7, 10 held


def _problem(sc, loss=None):
    P = FocalBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"], sc["focal_free"])
    P.set_loss(loss)
    return P


def _start(sc, x):
    """(rot_aa, cam_pos, focal, points) of the nodes x, as arrays of their own"""
    w, c, p = R.split(sc, x)
    return np.array(w), np.array(c), np.array(R.focal_of(sc, x)), np.array(p)


_ratio = R.ratio   # max |dev - hp| / (MARGIN max(max |fp64 - hp|, u max |hp|))


def _report(tag, worst):
    print("%-40s %s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _sv_reference(sc, lin, asm, radius, v):
    N = len(sc["cam_est"])
    dm = R.damped(sc, lin, asm, R.jacobi_scale(asm), radius)
    Sc, _, _ = R.schur_system(sc, dm)
    return (Sc @ v.reshape(-1).astype(Sc.dtype)).reshape(N, 7)   # (damped() puts the identity on inactive cameras and held focal coordinates)


# ---- 1. residuals, linearisation, Schur product ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(LOSSES))
@pytest.mark.parametrize("sname", ["a", "b", "c", "t"])
def test_linearisation_and_schur_product_against_hp_reference(sname, lname):
    sc = R.scene(sname)
    loss, kind, a = LOSSES[lname]
    N = len(sc["cam_est"])
    x = R.near_start(sname)
    w0, c0, f0, p0 = _start(sc, x)
    lin64, asm64 = R.point_linearisation(sname, kind, a, False)
    linhp, asmhp = R.point_linearisation(sname, kind, a, True)
    r64, rhp = R.point_observation(sname, False)[0], R.point_observation(sname, True)[0]
    P = _problem(sc, loss)
    r, rho = P.residuals(w0, c0, f0, p0)
    L = P.linearize(w0, c0, f0, p0)
    worst = {"r": _ratio(r, r64, rhp), "rho": _ratio(rho, lin64["rho"], linhp["rho"]), "cost": _ratio(L["cost"], asm64["cost"], asmhp["cost"]),
             "g_rot": _ratio(L["grad_rot"], asm64["g"][:N], asmhp["g"][:N]), "g_pos": _ratio(L["grad_pos"], asm64["g"][N:2 * N], asmhp["g"][N:2 * N]),
             "g_focal": _ratio(L["grad_focal"], asm64["g"][2 * N:3 * N, 0], asmhp["g"][2 * N:3 * N, 0]),
             "g_point": _ratio(L["grad_point"], asm64["g"][3 * N:], asmhp["g"][3 * N:]),
             "B": _ratio(L["diag_cam"], asm64["B"], asmhp["B"]), "B_focal": _ratio(L["diag_cam"][:, 6], asm64["B"][:, 6], asmhp["B"][:, 6]),
             "C": _ratio(L["diag_point"], asm64["C"], asmhp["C"])}
    assert np.all(r[~sc["used"]] == 0) and np.all(rho[~sc["used"]] == 0)
    ina = ~sc["cam_active"]
    assert np.all(L["diag_cam"][ina] == 0) and np.all(L["grad_rot"][ina] == 0) and np.all(L["grad_pos"][ina] == 0) and np.all(L["grad_focal"][ina] == 0)
    cut_case = sname == "t" and lname == "tukey"
    if cut_case:   # exact zeros on all 7 coordinates where every observation lies beyond the cut
        tp = sc["track_ptr"].astype(np.int64)
        rows = np.concatenate([np.flatnonzero(sc["obs_cam"] == CAM), np.arange(tp[TRK], tp[TRK + 1])])
        assert np.all(L["diag_cam"][CAM] == 0) and np.all(L["grad_rot"][CAM] == 0) and np.all(L["grad_pos"][CAM] == 0) and L["grad_focal"][CAM] == 0
        assert np.all(L["diag_point"][TRK] == 0) and np.all(L["grad_point"][TRK] == 0)
        assert np.all((r[rows] * r[rows]).sum(1) > 100.0)
    v = np.random.default_rng(3).standard_normal((N, 7))
    for radius in (1e4, 1e10):
        y64, yhp = _sv_reference(sc, lin64, asm64, radius, v), _sv_reference(sc, linhp, asmhp, radius, v)
        sv = P.schur_matvec(v, radius)
        worst["Sv@%.0e" % radius] = _ratio(sv, y64, yhp)
        worst["Sv_focal@%.0e" % radius] = _ratio(sv[:, 6], y64[:, 6], yhp[:, 6])
        assert np.array_equal(sv[ina], v[ina])
        if cut_case:   # S reduces to the damping on camera 4's rows
            worst["Sv_cam%d@%.0e" % (CAM, radius)] = _ratio(sv[CAM], y64[CAM], yhp[CAM])
    _report("%s %s" % (sname, lname), worst)


# ---- 2. one LM step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e4, 1e10])
@pytest.mark.parametrize("sname", ["a", "b", "c"])
def test_step_against_refined_hp_solution(sname, radius):
    _step(sname, "huber", radius)


@pytest.mark.parametrize("sname,lname,radius", [("t", "tukey", 1e4), ("t", "tukey", 1e10), ("a", "geman", 1e4)])
def test_step_under_tukey_and_geman_mcclure(sname, lname, radius):
    """Scene t under Tukey: a camera (all 7 coordinates) and a point whose blocks are the damping alone; [t-tukey-1e10] is the case
    k_fba_cam_precond's second tier exists for (test_gpu_ba6.py's test of the same name).

    [t-tukey-1e10], at the default options like every case here, is also what gsfm_ba7_options_default's stall rule comes from.  More than
    half of the scene's observations are beyond the cut and the damping is 1e-16 to 1e-10 of the blocks; the preconditioned reduced system
    has the seven gauge directions as eigenvalues 5e-10 to 1e-7 (as gsfm_ba6's has) and 19 eigenvalues below 0.1 where gsfm_ba6's has 13.
    A float64 block-Jacobi PCG on the reference's own matrix needs 710 to 950 iterations (gsfm_ba6's system: 490 to 530) with runs of 110 to
    230 iterations in which r.M^-1 r is not quartered -- whether the block inverses are numpy's, the Cholesky-Gram inverses the device forms,
    or Cholesky solves (the inverse's accuracy is not the cause) -- and an MI355X needs 1600.  With gsfm_ba6's cg_stall_iterations = 200 the
    device gave up at 696 iterations (relative residual 1.1e-6; from a 2 per cent focal perturbation at 568, 4.9e-7); the default is now half
    of max_cg_iterations (include/gsfm_ba7.h)."""
    _step(sname, lname, radius)


@pytest.mark.parametrize("radius", [1e4, 1e10])
def test_preconditioner_applied_to_the_right_hand_side_matches_the_hp_blocks(radius):
    """Scene t under Tukey, per camera: after ONE PCG iteration y_c = alpha M^-1 rhs with one scalar alpha for all cameras, so y_c / alpha is
    k_fba_cam_precond's block inverse applied to the row's right-hand side -- rows that take its second tier (the plain-fp64 block
    indefinite) included.  Compared row by row with the hp tier's Schur-Jacobi block solved in long double.  alpha is the median of the
    entrywise quotients (a least-squares fit would carry the ill-conditioned rows' errors into every row).
    Bound per row: MARGIN x the larger of the fp64 tier's own deviation (its block, solved by elimination in float64) and
    u cond_2(M_k) max |z_k|.  The second term is what an explicit inverse costs: the device forms M_k^-1 = L^-T L^-1 and multiplies, whose
    forward error is of order u cond(M_k) where a solve's is often far smaller; for a preconditioner that is no loss -- any fixed symmetric
    positive definite operator near M^-1 serves, and the host PCG of DESIGN.md section 19 needs the same iterations with either -- so the
    check is that each row's operator IS the Schur-Jacobi block to that accuracy, not the block of B~ alone or a failed factorisation.  The
    rows' relative deviations and the rows whose bound says nothing (u cond > 1e-3) are printed."""
    sc = R.scene("t")
    N = len(sc["cam_est"])
    w0, c0, f0, p0 = _start(sc, R.near_start("t"))
    P = _problem(sc, LOSSES["tukey"][0])
    st = P.step_check(w0, c0, f0, p0, radius, max_cg_iterations=1, cg_check_interval=1)
    assert st["cg_iterations"] == 1
    z, rhs = {}, {}
    for hp in (False, True):
        lin, asm = R.point_linearisation("t", *B.TUKEY, hp)
        _, b, Mb = R.schur_system(sc, R.damped(sc, lin, asm, R.jacobi_scale(asm), radius))
        rhs[hp] = b.reshape(N, 7)
        z[hp] = np.array([R._solve_small(Mb[k], rhs[hp][k]) for k in range(N)])
    cond = np.array([np.linalg.cond(np.asarray(m, np.float64)) for m in Mb])   # (of the hp tier's blocks)
    z64, zhp = z[False], np.asarray(z[True], R.LD)
    y = st["y_cam"]
    big = np.abs(zhp) > 1e-3 * np.abs(zhp).max(1, keepdims=True)
    alpha = float(np.median((y / np.where(big, zhp, 1).astype(float))[big & (zhp != 0)]))
    worst = {"rhs": _ratio(st["rhs"], rhs[False], rhs[True])}
    rows, rel = {}, {}
    for k in np.flatnonzero(sc["cam_active"]):
        scale = float(np.abs(zhp[k]).max())
        if scale == 0:
            continue
        e_dev = float(np.abs(np.asarray(y[k] / alpha, R.LD) - zhp[k]).max())
        e_ref = float(np.abs(np.asarray(z64[k], R.LD) - zhp[k]).max())
        rows[k] = e_dev / (R.MARGIN * max(e_ref, R.U * max(1.0, cond[k]) * scale))
        rel[k] = e_dev / scale
    k_worst = max(rows, key=rows.get)
    worst["M^-1 rhs, worst row (camera %d)" % k_worst] = rows[k_worst]
    silent = sorted(int(k) for k in rows if R.U * cond[k] > 1e-3)
    told = [k for k in rows if k not in silent]
    print("radius %.0e: alpha %.12e, %d rows; relative deviation median %.2e, max %.2e (camera %d, cond %.1e) over the %d rows with u cond <= 1e-3; rows whose bound says nothing: %s (deviations %s)"
          % (radius, alpha, len(rows), np.median([rel[k] for k in told]), max(rel[k] for k in told), max(told, key=rel.get), cond[max(told, key=rel.get)], len(told), silent,
             ["%.1e" % rel[k] for k in silent]))
    assert np.all(y[CAM] == 0) and len(told) >= 50   # the cut camera: zero right-hand side
    _report("t tukey preconditioner radius %.0e" % radius, worst)


def test_step_with_a_mixed_focal_mask_holds_the_held_focal_lengths():
    _step("a", "huber", 1e4, MIXED)


def _step(sname, lname, radius, focal_free=None):
    sc = R.scene(sname, focal_free)
    N = len(sc["cam_est"])
    x = R.near_start(sname)
    w0, c0, f0, p0 = _start(sc, x)
    loss, kind, a = LOSSES[lname]
    P = _problem(sc, loss)
    st = P.step_check(w0, c0, f0, p0, radius)
    off = P.step_check(w0, c0, f0, p0, radius, remove_gauge=0)
    if sname == "t" and lname == "tukey":   # zero gradient, zero coupling: y = 0 there
        assert np.all(off["delta_rot"][CAM] == 0) and np.all(off["delta_pos"][CAM] == 0) and off["delta_focal"][CAM] == 0 and np.all(off["delta_point"][TRK] == 0)
    tiers = {}
    for hp in (False, True):
        lin, asm = R.point_linearisation(sname, kind, a, hp, focal_free)
        y, dm = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), radius, hp=hp)
        xt = x.astype(y.dtype)
        jl = R.jl_hp(sc, x) if hp else None
        t = dict(lin=lin, asm=asm, y=y, dm=dm, rhs=R.schur_system(sc, dm)[1].reshape(N, 7))
        for key, gauge in (("delta", True), ("plain", False)):
            d = R.project_step(sc, dm, y, xt, gauge, jl)
            t[key], t["jd_" + key] = d, R.apply_J(sc, lin, d)
            t["model_" + key] = -(d * asm["g"]).sum() - (t["jd_" + key] ** 2).sum() / 2
        tiers[hp] = t
    lo, hi = tiers[False], tiers[True]
    rel, floor = R.pcg_residual_and_floor(sc, hi["dm"], st["y_cam"])
    print("%s radius %.0e: PCG %d iterations, recursion residual %.2e, true residual %.2e, floor %.2e" % (sname, radius, st["cg_iterations"], st["cg_rel"], rel, floor))
    tol = P.default_options().cg_relative_tolerance   # (gsfm_ba7_options_default: 1e-14)
    assert tol == 1e-14 and not st["stalled"] and not off["stalled"] and st["cg_rel"] <= tol
    assert rel <= tol + floor
    yp_hp = R.back_substitute(sc, hi["dm"], np.asarray(st["y_cam"], R.LD).reshape(-1))
    yp_64 = R.back_substitute(sc, lo["dm"], np.asarray(st["y_cam"], np.float64).reshape(-1))

    def dev_nodes(s):
        return R.nodes(s["delta_rot"], s["delta_pos"], s["delta_focal"], s["delta_point"])
    dev_delta = dev_nodes(st)
    worst = {"rhs": _ratio(st["rhs"], lo["rhs"], hi["rhs"]), "y_point": _ratio(st["y_point"], yp_64, yp_hp),
             "model": _ratio(st["model_cost_change"], lo["model_delta"], hi["model_delta"]),
             "J_delta": _ratio(st["j_delta"], lo["jd_delta"], hi["jd_delta"]),
             "model_plain": _ratio(off["model_cost_change"], lo["model_plain"], hi["model_plain"]),
             "J_delta_plain": _ratio(off["j_delta"], lo["jd_plain"], hi["jd_plain"])}
    if radius == 1e4:   # (at 1e10 delta itself is decided by the conditioning of the damping: test_gpu_ba6.py)
        worst["delta"] = _ratio(dev_delta, lo["delta"], hi["delta"])
        worst["delta_focal"] = _ratio(st["delta_focal"], R.focal_of(sc, lo["delta"]), R.focal_of(sc, hi["delta"]))
        worst["delta_plain"] = _ratio(dev_nodes(off), lo["plain"], hi["plain"])
    act = hi["dm"]["act"]
    dn = np.sqrt((dev_delta * dev_delta).sum())
    d64 = np.asarray(lo["delta"], np.float64)
    for i, v in enumerate(R.gauge_directions(sc, x)):
        vn = np.sqrt((v * v).sum())
        kept64 = abs((d64 * v).sum()) / (np.sqrt((d64 * d64).sum()) * vn)
        kept = abs((dev_delta * v).sum()) / (dn * vn)
        worst["gauge%d" % i] = kept / (R.MARGIN * max(kept64, R.U))
    assert np.all(dev_delta[~act] == 0)   # inactive nodes and held focal lengths: exactly 0
    if focal_free is not None:
        held = sc["cam_active"] & ~sc["focal_free"]
        assert held.any() and np.all(st["delta_focal"][held] == 0) and np.all(st["delta_focal"][sc["cam_active"] & sc["focal_free"]] != 0)
        assert np.all(st["rhs"][held, 6] == 0) and np.all(st["y_cam"][held, 6] == 0)
    assert abs(float(hi["model_plain"]) - float(hi["model_delta"])) <= 1e-9 * float(hi["model_delta"])   # (the reference's own: J V = 0)
    _report("%s %s step radius %.0e" % (sname, lname, radius), worst)


# ---- 3. full solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["a0", "b0", "c0"])
def test_noise_free_observations_bring_the_cost_to_the_stopping_rules_level(sname):
    """No bound on the recovered scene is derived here: the solve stops at a step of 1e-8 (|x| + 1e-8), and |x| is dominated by the focal
    lengths (sqrt(N) x 1e3 pixels), so the last step may be 1e-5 long in coordinates where centres and points are of order one; what that
    leaves of the error depends on the conditioning of the scene, which no argument here bounds.  What the stopping rules do give: the
    minimum is 0, so a solve that ends by a tolerance with more than function_tolerance of its initial cost left has not converged.
    Recovery itself is the comparison with the hp tier (test_noisy_solve_matches_the_reference); the error is printed."""
    sc = R.scene(sname)
    w0, c0, f0, p0 = _start(sc, R.near_start(sname))
    w1, c1, f1, p1, s = _problem(sc).solve(w0, c0, f0, p0)
    got = R.aligned(sc, R.nodes(w1, c1, f1, p1), R.nodes(sc["rot_aa"], sc["cam_pos"], sc["intrinsics"][:, 0], sc["gt_points"]))
    want = R.aligned(sc, R.nodes(sc["rot_aa"], sc["cam_pos"], sc["intrinsics"][:, 0], sc["gt_points"]), R.nodes(sc["rot_aa"], sc["cam_pos"], sc["intrinsics"][:, 0], sc["gt_points"]))
    nf = int(sc["cam_active"].sum())
    print(sname, s["termination_name"], s["num_iterations"], "cost %.3e -> %.3e" % (s["initial_cost"], s["final_cost"]), "scene error %.3e" % np.abs(got - want)[:-nf].max(),
          "relative focal error %.3e" % np.abs(got[-nf:] / want[-nf:] - 1).max(), "cg", s["num_cg_iterations"])
    assert s["termination"] in (0, 1, 2) and s["num_pcg_stalled_steps"] == 0
    assert s["final_cost"] <= 1e-6 * s["initial_cost"]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_noisy_solve_matches_the_reference(name):
    sc = R.scene(R.CASES[name][0])
    x0 = R.case_start(name)
    w0, c0, f0, p0 = _start(sc, x0)
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    w1, c1, f1, p1, s = _problem(sc, LOSSES[CASE_LOSS[R.case_loss(name)]][0]).solve(w0, c0, f0, p0)
    print(name, s["termination_name"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], "cg", s["num_cg_iterations"],
          "stalled", s["num_pcg_stalled_steps"], "cost %.15e (hp %.15e)" % (s["final_cost"], hi["final_cost"]))
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"]) == \
        (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert s["num_pcg_stalled_steps"] == 0
    al = lambda xx: R.aligned(sc, xx, hi["x"])   # one alignment, onto the hp tier's result, for the device and both tiers
    dev = R.nodes(w1, c1, f1, p1)
    nf = int(sc["cam_active"].sum())
    worst = {"initial_cost": _ratio(s["initial_cost"], lo["initial_cost"], hi["initial_cost"]), "final_cost": _ratio(s["final_cost"], lo["final_cost"], hi["final_cost"]),
             "x": _ratio(al(dev), al(lo["x"]), al(hi["x"])), "focal": _ratio(al(dev)[-nf:], al(lo["x"])[-nf:], al(hi["x"])[-nf:])}
    assert not np.array_equal(f1[sc["cam_active"]], f0[sc["cam_active"]])
    _report(name, worst)


# ---- 4. the rest ---------------------------------------------------------------------------------------------------------------
def test_two_solves_return_the_same_bytes_and_inactive_nodes_pass_bit_for_bit():
    sc = R.scene("a")
    w0, c0, f0, p0 = _start(sc, R.case_start("a_near"))
    odd = np.array([-0.0, np.nan, 1e300])
    ina = ~sc["cam_active"]
    w0[ina] = odd
    c0[ina] = odd[::-1]
    f0[ina] = np.resize(odd, ina.sum())
    p0[~sc["pt_active"]] = odd
    assert ina.sum() >= 1 and (~sc["pt_active"]).sum() >= 3
    P = _problem(sc, LOSSES["huber"][0])
    one = P.solve(w0, c0, f0, p0)
    two = P.solve(w0, c0, f0, p0)
    three = bundle_adjust_focal(w0, c0, f0, sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], p0, sc["cam_est"], sc["pt_est"], loss=LOSSES["huber"][0])
    for k in range(4):
        assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes()
    assert one[4]["final_cost"] == two[4]["final_cost"] == three[4]["final_cost"] and one[4]["num_cg_iterations"] == two[4]["num_cg_iterations"]
    w1, c1, f1, p1, s1 = one
    assert w1[ina].tobytes() == w0[ina].tobytes() and c1[ina].tobytes() == c0[ina].tobytes() and f1[ina].tobytes() == f0[ina].tobytes()
    assert p1[~sc["pt_active"]].tobytes() == p0[~sc["pt_active"]].tobytes()
    for got, start in ((w1, w0), (c1, c0), (f1, f0)):
        assert np.all(np.isfinite(got[sc["cam_active"]])) and not np.any(got[sc["cam_active"]] == start[sc["cam_active"]])
    assert (s1["num_observations_used"], s1["num_active_cameras"], s1["num_active_points"]) == (sc["used"].sum(), sc["cam_active"].sum(), sc["pt_active"].sum())


def test_a_mixed_focal_mask_returns_held_focal_lengths_bit_for_bit_and_moves_the_others():
    sc = R.scene("a", MIXED)
    w0, c0, f0, p0 = _start(sc, R.case_start("a_near"))
    w1, c1, f1, p1, s = _problem(sc, LOSSES["huber"][0]).solve(w0, c0, f0, p0)
    held, free = ~MIXED, MIXED & sc["cam_active"]
    assert s["termination"] in (0, 1, 2) and s["final_cost"] < s["initial_cost"] and s["num_pcg_stalled_steps"] == 0
    assert (held & sc["cam_active"]).sum() >= 3 and f1[held].tobytes() == f0[held].tobytes() and np.all(f1[free] != f0[free])
    assert not np.array_equal(w1[held & sc["cam_active"]], w0[held & sc["cam_active"]])   # (the rest of a held camera is adjusted)
    lo, hi = [R.lm_solve(sc, R.case_start("a_near"), *R.LOSS, hp=hp) for hp in (False, True)]
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"]) == (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    al = lambda xx: R.aligned(sc, xx, hi["x"])
    _report("a_near mixed mask", {"x": _ratio(al(R.nodes(w1, c1, f1, p1)), al(lo["x"]), al(hi["x"]))})


def test_all_focal_lengths_held_is_the_six_coordinate_adjustment():
    """focal_free all zero from ba6_reference's a_near start with the generator's focal lengths: ba6_reference's result within the bound, and
    the termination and counts of its hp tier"""
    sc = R6.scene("a")
    w0, c0, p0 = R6.split(sc, R6.case_start("a_near"))
    f0 = sc["intrinsics"][:, 0].copy()
    lo, hi = R6.case_solve("a_near", False), R6.case_solve("a_near", True)
    P = FocalBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], sc["cam_est"], sc["pt_est"], np.zeros(12, np.uint8))
    P.set_loss(LOSSES["huber"][0])
    w1, c1, f1, p1, s = P.solve(w0, c0, f0, p0)
    assert f1.tobytes() == f0.tobytes()
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"]) == (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    al = lambda w, c, p: R6.align(sc, w, c, p, hi["cam"], hi["points"])
    _report("a_near, all held", {"final_cost": _ratio(s["final_cost"], lo["final_cost"], hi["final_cost"]),
                                 "x": _ratio(al(w1, c1, p1), al(lo["rot"], lo["cam"], lo["points"]), al(hi["rot"], hi["cam"], hi["points"]))})


def test_a_problem_without_a_used_observation_changes_nothing():
    sc = R.scene("a")
    w0, c0, f0, p0 = _start(sc, R.case_start("a_near"))
    P = FocalBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], np.zeros(12, np.uint8), None)
    w1, c1, f1, p1, s = P.solve(w0, c0, f0, p0)
    assert w1.tobytes() == w0.tobytes() and c1.tobytes() == c0.tobytes() and f1.tobytes() == f0.tobytes() and p1.tobytes() == p0.tobytes()
    assert s["num_observations_used"] == 0 and s["num_iterations"] == 0
    P = FocalBundleProblem(sc["intrinsics"], np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 2)))
    w1, c1, f1, p1, s = P.solve(w0, c0, f0, np.zeros((0, 3)))
    assert w1.tobytes() == w0.tobytes() and f1.tobytes() == f0.tobytes() and s["num_observations_used"] == 0


def test_argument_and_loss_errors():
    sc = R.scene("a")
    P = _problem(sc)
    w0, c0, f0, p0 = _start(sc, R.near_start("a"))
    for nodes in ([(_abi.LOSS_MAGSAC, 0.02, 9.0, 0.0)], [(1, 10.0, 0, 0), (1, 10.0, 0, 0)], [(1, -1.0, 0, 0)], [(_abi.LOSS_CAUCHY, 10.0, 0, 0)],
                  [(_abi.LOSS_TUKEY, 0.0, 0, 0)], [(_abi.LOSS_GEMAN_MCCLURE, 10.0, float("inf"), 0)]):
        with pytest.raises(SolverError, match="status 1"):
            P.set_loss(nodes)
    P.set_loss(LF.TukeyLoss(10.0))
    P.set_loss(LF.GemanMcClureLoss(10.0, 0.5))
    with pytest.raises(SolverError, match="status 1"):
        P.schur_matvec(np.zeros((12, 7)))   # no linearisation yet
    with pytest.raises(SolverError, match="status 1"):
        P.step_check(w0, c0, f0, p0, radius=0.0)
    # a focal length that is not finite or not positive on an active camera, free or held; an inactive camera may carry anything
    active = int(np.flatnonzero(sc["cam_active"])[0])
    Ph = _problem(R.scene("a", np.zeros(12, bool)))
    for bad in (0.0, -1000.0, float("nan"), float("inf")):
        f = f0.copy()
        f[active] = bad
        for prob in (P, Ph):
            for call in (lambda q: q.solve(w0, c0, f, p0), lambda q: q.linearize(w0, c0, f, p0), lambda q: q.step_check(w0, c0, f, p0)):
                with pytest.raises(SolverError, match="status 1.*focal length"):
                    call(prob)
    inactive = int(np.flatnonzero(~sc["cam_active"])[0])
    f = f0.copy()
    f[inactive] = float("nan")
    out = P.solve(w0, c0, f, p0)
    assert np.isnan(out[2][inactive]) and out[4]["termination"] in (0, 1, 2)
    with pytest.raises(ValueError):
        FocalBundleProblem(sc["intrinsics"], sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], focal_free=np.ones(5))


@pytest.mark.parametrize("name", ["a_near", "a_far", "a_near_mixed"])
def test_focal_solve_keeps_the_bytes_of_the_commit_before_the_shared_kernel_family(name):
    """gsfm_ba7_solve under Huber 10 from case_start (a_near_mixed: a_near with the MIXED focal mask): the bytes and counts recorded on an
    MI355X from a library built from the commit before the 6- and 7-coordinate solvers became one kernel family and one host template
    (tools/make_full_ba_parent_golden.py, tests/golden/ba7_solve_parent_bytes.npz).  The far start takes rejected steps."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba7_solve_parent_bytes.npz"))
    case = "a_near" if name == "a_near_mixed" else name
    sc = R.scene(R.CASES[case][0], MIXED if name == "a_near_mixed" else None)
    w1, c1, f1, p1, s = _problem(sc, LOSSES["huber"][0]).solve(*_start(sc, R.case_start(case)))
    counts = [s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], s["num_cg_iterations"]]
    print(name, counts, "final cost %.17g" % s["final_cost"])
    if name == "a_far":
        assert str(gold["far_case"]) == name and gold[name + "_counts"][3] > 0
    for key, got in (("rot", w1), ("cam", c1), ("focal", f1), ("points", p1)):
        assert got.tobytes() == gold[name + "_" + key].tobytes(), key
    assert s["final_cost"] == gold[name + "_final_cost"][0]
    assert counts == list(gold[name + "_counts"])
