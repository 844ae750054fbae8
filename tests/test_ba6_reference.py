"""CPU: the reference of the full bundle adjustment (tests/ba6_reference.py) checked against itself, and the conditions on the inputs of
tests/test_gpu_ba6.py."""
import mpmath
import numpy as np
import pytest

import ba6_reference as R

SCENES = ["a", "b", "c"]


def test_scene_c_has_the_chosen_orientations():
    sc = R.scene("c")
    th = np.linalg.norm(sc["rot_aa"][:5], axis=1)
    assert th[0] == 0.0 and np.allclose(th[1:], R.C_ANGLES[1:], rtol=1e-12)
    assert th[2] ** 2 < 1e-2 < th[3] ** 2     # either side of jl_and_inverse's branch
    assert sc["cam_active"][:5].all() and sc["used"].sum() > 100
    # the cameras look at the cloud: every used observation has positive depth
    x = R.nodes(sc["rot_aa"], sc["cam_pos"], sc["gt_points"])
    rot, cam, pts = R.split(sc, x)
    from globalsfmpy_amd import synth
    p = np.einsum("eij,ej->ei", synth.aa_to_matrix(rot)[sc["obs_cam"]], pts[sc["track_of"]] - cam[sc["obs_cam"]])
    assert (p[sc["used"], 2] > 1.0).all()


def test_left_jacobian_series_meets_the_closed_form_at_40_digits():
    with mpmath.workdps(R.MP_DPS):
        for t in (R.JL_SERIES_BELOW, 0.5 * R.JL_SERIES_BELOW, 1e-9):
            t2 = mpmath.mpf(t) ** 2
            a_s, b_s = R.jl_coefficients_mp(t2, True)
            with mpmath.workdps(3 * R.MP_DPS):   # (the closed forms cancel: evaluate them with digits to spare)
                a_c, b_c = R.jl_coefficients_mp(t2, False)
            assert abs(a_s - a_c) <= mpmath.mpf(10) ** (-R.MP_DPS + 2) and abs(b_s - b_c) <= mpmath.mpf(10) ** (-R.MP_DPS + 2)
        # and the closed form at the working precision, just above the threshold, keeps 30 digits
        t2 = mpmath.mpf(R.JL_SERIES_BELOW) ** 2
        a_w, b_w = R.jl_coefficients_mp(t2, False)
        a_s, b_s = R.jl_coefficients_mp(t2, True)
        assert abs(a_w - a_s) <= mpmath.mpf(10) ** -30 and abs(b_w - b_s) <= mpmath.mpf(10) ** -27
    # the float64 tier's J_l against the hp tier's, over scene c's orientations and a few more
    ws = np.concatenate([R.scene("c")["rot_aa"], [[0.006, 0.006, 0.006], [0.0058, -0.0058, 0.0057], [1.0, -2.0, 0.5]]])
    with mpmath.workdps(R.MP_DPS):
        hp = np.array([[[float(v) for v in row] for row in R.left_jacobian_mp(w)] for w in ws])
    assert np.abs(R.left_jacobian_np(ws) - hp).max() <= 8 * R.U


@pytest.mark.parametrize("sname", ["a", "c"])
def test_jacobian_against_central_differences_of_the_hp_residual(sname):
    sc = R.scene(sname)
    x = R.near_start(sname)
    _, Jp, Jr = R.observe_np(sc, x)
    N = len(sc["cam_est"])
    cams = [0, 1, 2, 3, 4] if sname == "c" else [0, 7]
    h = 2.0 ** -20
    worst = 0.0
    for k in cams:
        es = np.flatnonzero(sc["used"] & (sc["obs_cam"] == k))[:3]
        for node, J in ((k, Jr), (N + k, -Jp)):
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[node, c] += h
                xm[node, c] -= h
                d = (R.residual_hp(sc, xp)[es] - R.residual_hp(sc, xm)[es]) / R.LD(2 * h)
                worst = max(worst, float(np.abs(d - J[es, :, c]).max() / np.abs(J[es]).max()))
    # a point, through one of its observations
    t = int(sc["track_of"][np.flatnonzero(sc["used"])[0]])
    es = np.flatnonzero(sc["used"] & (sc["track_of"] == t))
    for c in range(3):
        xp, xm = x.copy(), x.copy()
        xp[2 * N + t, c] += h
        xm[2 * N + t, c] -= h
        d = (R.residual_hp(sc, xp)[es] - R.residual_hp(sc, xm)[es]) / R.LD(2 * h)
        worst = max(worst, float(np.abs(d - Jp[es, :, c]).max() / np.abs(Jp[es]).max()))
    print(sname, "central differences: worst relative deviation %.2e" % worst)
    assert worst <= 1e-9   # (the truncation error of the difference quotient, h^2 times the third derivative, is of order 1e-11)


@pytest.mark.parametrize("sname", SCENES)
def test_all_seven_gauge_directions_are_null_vectors_of_the_jacobian(sname):
    sc = R.scene(sname)
    x = R.near_start(sname)
    lin, _ = R.point_linearisation(sname, "huber", 10.0, False)
    scale = np.abs(lin["Jc"]).max()
    for i, v in enumerate(R.gauge_directions(sc, x)):
        jv = np.abs(R.apply_J(sc, lin, v)).max()
        assert jv <= 1e-9 * scale * np.abs(v).max(), (i, jv, scale)
    assert len(R.gauge_directions(sc, x)) == 7


@pytest.mark.parametrize("radius", [1e4, 1e10])
def test_reduced_solve_equals_the_full_solve_and_the_projection_keeps_the_model(radius):
    sc = R.scene("a")
    x = R.near_start("a")
    lin, asm = R.point_linearisation("a", "huber", 10.0, False)
    S = R.jacobi_scale(asm)
    y_full, dm = R.solve_step(sc, lin, asm, S, radius)
    Sc, rhs, _ = R.schur_system(sc, dm)
    yc = np.linalg.solve(Sc, rhs)
    y_red = np.concatenate([R.cam6_to_nodes(yc), R.back_substitute(sc, dm, yc)])
    if radius == 1e4:
        assert np.abs(y_red - y_full).max() <= 1e-6 * np.abs(y_full).max()
    # (at 1e10 the gauge part of y is set by the damping alone, eleven digits below the rest: compare what the gauge does not touch)
    jd = [R.apply_J(sc, lin, np.where(dm["act"][:, None], -S * y, 0)) for y in (y_red, y_full)]
    assert np.abs(jd[0] - jd[1]).max() <= 1e-6 * np.abs(jd[1]).max()
    models = []
    for gauge in (True, False):
        d = R.project_step(sc, dm, y_full, x, gauge)
        models.append(-(d * asm["g"]).sum() - R.quad_form(sc, lin, d) / 2)
    assert abs(models[0] - models[1]) <= 1e-9 * abs(models[1])
    d = R.project_step(sc, dm, y_full, x, True)
    for v in R.gauge_directions(sc, x):
        assert abs((d * v).sum()) <= 1e-10 * np.sqrt((d * d).sum() * (v * v).sum())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_conditions_on_the_cases_of_the_gpu_tests(name):
    """Both tiers take the same LM decisions, and no comparison lies within 1e-6 (relative) of its threshold: a condition on the inputs
    (the start seeds of ba6_reference.CASES were chosen for it), not a tolerance."""
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    print(name, R.TERM_NAMES[hi["termination"]], hi["iterations"], hi["successful"], hi["unsuccessful"], "cost %.6e -> %.6e" % (hi["initial_cost"], hi["final_cost"]),
          "margin %.2e" % R.decision_margin(hi["decisions"]))
    assert (lo["termination"], lo["iterations"], lo["successful"], lo["unsuccessful"]) == (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert [d[0] for d in lo["decisions"]] == [d[0] for d in hi["decisions"]]
    assert hi["termination"] in (0, 1, 2)
    assert R.decision_margin(hi["decisions"]) > 1e-6 and R.decision_margin(lo["decisions"]) > 1e-6
    if name.endswith("far"):
        assert hi["unsuccessful"] >= 1
    assert hi["final_cost"] < hi["initial_cost"]


@pytest.mark.parametrize("sname", ["a0", "c0"])
def test_noise_free_scenes_end_at_the_generator_scene(sname):
    sc = R.scene(sname)
    out = R.lm_solve(sc, R.near_start(sname))
    got = R.align(sc, out["rot"], out["cam"], out["points"], sc["cam_pos"], sc["gt_points"])
    want = R.align(sc, sc["rot_aa"], sc["cam_pos"], sc["gt_points"], sc["cam_pos"], sc["gt_points"])
    err = np.abs(got - want).max()
    print(sname, R.TERM_NAMES[out["termination"]], out["iterations"], "final cost %.3e" % out["final_cost"], "error %.3e" % err)
    assert out["termination"] in (0, 1, 2) and err <= 1e-6


# ---- Tukey and Geman-McClure ---------------------------------------------------------------------------------------------------------
def test_corrector_matches_the_robustified_cost_for_every_loss():
    """J~^T r~ = rho' J^T r on the camera (6) and the point (3) side, for both Huber branches, SoftLOne, both Tukey branches and Geman-McClure."""
    sc = R.scene("a")
    r, Jp, Jr = R.point_observation("a", False)
    for kind, a in (("huber", 10.0), ("softl1", 10.0), R.B.TUKEY, R.B.GEMAN):
        with np.errstate(all="raise"):   # (finite where used: nothing the reference keeps divides by rho' = 0)
            lin = R.linearise(r, Jp, Jr, kind, a)
        _, rho1, _ = R.loss_rho(kind, a, lin["s"])
        for got, J in ((np.einsum("eki,ek->ei", lin["Jc"], lin["rt"]), np.concatenate([Jr, -Jp], 2)), (np.einsum("eki,ek->ei", lin["Jp"], lin["rt"]), Jp)):
            want = rho1[:, None] * np.einsum("eki,ek->ei", J, r)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    s = R.linearise(r, Jp, Jr, *R.B.TUKEY)["s"][sc["used"]]
    assert (s > 100.0).any() and (s <= 100.0).any()


@pytest.mark.parametrize("hp", [False, True])
def test_scene_t_conditions_under_tukey(hp):
    """What tests/test_gpu_ba6.py asserts as exact zeros holds on the reference's own lin / asm at the near start, in both tiers."""
    sc = R.scene("t")
    N = len(sc["cam_est"])
    cam, trk = R.B.T_CAMERA, R.B.T_TRACK
    lin, asm = R.point_linearisation("t", *R.B.TUKEY, hp)
    tp = sc["track_ptr"].astype(np.int64)
    s = lin["s"]
    cam_rows, track_rows = np.flatnonzero(sc["obs_cam"] == cam), np.arange(tp[trk], tp[trk + 1])
    assert len(cam_rows) == 3 and len(track_rows) == 2 and sc["used"].all()
    assert np.all(s[cam_rows] > 100.0) and np.all(s[track_rows] > 100.0) and all(s[tp[t] + k] > 100.0 for t, k in R.B.T_SINGLE)
    assert np.all(asm["B"][cam] == 0) and np.all(asm["C"][trk] == 0)                                  # exactly
    assert np.all(asm["g"][[cam, N + cam, 2 * N + trk]] == 0)
    assert np.all(lin["rho"][np.concatenate([cam_rows, track_rows])] == lin["rho"].dtype.type(100) / 6)
    others = np.setdiff1d(np.arange(len(s)), np.concatenate([cam_rows, track_rows]))
    assert (s[others] > 100.0).any() and (s[others] <= 100.0).any()                                   # both branches among the rest
    n = np.sqrt(np.asarray(s, np.float64))
    assert ((n > 9.9) & (n <= 10.0)).any() and ((n > 10.0) & (n < 10.1)).any()                        # within 1 % of the cut, on either side
    for radius in (1e4, 1e10):
        y, dm = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), radius, hp=hp)
        d2 = dm["S"].dtype.type(R.DEFAULTS["min_lm_diagonal"]) / dm["S"].dtype.type(radius)
        assert np.all(dm["Bt"][cam] == d2 * np.eye(6)) and np.all(dm["Ct"][trk] == d2 * np.eye(3))    # the clamp alone, Jacobi scale 1 / (1 + 0)
        Sc = R.schur_system(sc, dm)[0]
        rows = slice(6 * cam, 6 * cam + 6)
        assert np.all(Sc[rows, rows] == d2 * np.eye(6)) and np.count_nonzero(Sc[rows]) == 6           # S reduces to the damping there
        plain = R.project_step(sc, dm, y, np.zeros_like(y), gauge=False)
        assert np.all(plain[[cam, N + cam, 2 * N + trk]] == 0)                                        # the plain step leaves them where they are


def test_cut_camera_and_track_of_scene_t_through_a_solve():
    """tests/test_ba_reference.py's test of the same name: with the gauge projection camera 4 (orientation and centre) and track 5 move, without
    it they keep their input bytes; their observations are beyond the cut at the end as at the start."""
    sc = R.scene("t")
    N = len(sc["cam_est"])
    x0 = R.case_start("t_near_tukey")
    idx = [R.B.T_CAMERA, N + R.B.T_CAMERA, 2 * N + R.B.T_TRACK]
    for o, moved in ((R.case_solve("t_near_tukey", False), True), (R.lm_solve(sc, x0, *R.B.TUKEY, remove_gauge=0), False)):
        asm = R.assemble(sc, R.linearise(*R.observe_np(sc, o["x"]), *R.B.TUKEY))
        assert np.all(asm["B"][R.B.T_CAMERA] == 0) and np.all(asm["C"][R.B.T_TRACK] == 0)
        assert o["termination"] in (0, 1, 2) and o["iterations"] >= 3
        assert [o["x"][i].tobytes() != x0[i].tobytes() for i in idx] == [moved] * 3


@pytest.mark.parametrize("name", sorted(R.B.DEFECTS))
def test_a_defective_loss_exceeds_the_bound_of_the_gpu_tests(name):
    """tests/test_ba_reference.py's test of the same name, on the full adjustment's linearisation (scene a, near start)."""
    kind, a = R.B.DEFECTS[name]
    sc = R.scene("a")
    N = len(sc["cam_est"])
    _, asm64 = R.point_linearisation("a", kind, a, False)
    _, asmhp = R.point_linearisation("a", kind, a, True)
    with R.B.defect(name):
        bad = R.assemble(sc, R.linearise(*R.point_observation("a", False), kind, a))
    worst = {"g_rot": R.ratio(bad["g"][:N], asm64["g"][:N], asmhp["g"][:N]), "g_pos": R.ratio(bad["g"][N:2 * N], asm64["g"][N:2 * N], asmhp["g"][N:2 * N]),
             "g_point": R.ratio(bad["g"][2 * N:], asm64["g"][2 * N:], asmhp["g"][2 * N:]), "B": R.ratio(bad["B"], asm64["B"], asmhp["B"]),
             "C": R.ratio(bad["C"], asm64["C"], asmhp["C"])}
    print(name, worst)
    assert min(worst.values()) > 1.0
    assert R.ratio(asm64["g"], asm64["g"], asmhp["g"]) <= 1.0 / R.MARGIN     # (and the same arithmetic without the defect is inside it)
