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
