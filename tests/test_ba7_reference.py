"""tests/ba7_reference.py checked against itself and against tests/ba6_reference.py on the CPU: the seventh coordinate's Jacobian against
central differences of the 40-digit residual, the gauge, the six-coordinate problem as the special case focal_free = 0, and the conditions
the GPU tests (tests/test_gpu_ba7.py) put on their cases."""
import numpy as np
import pytest

import ba_reference as B
import ba6_reference as R6
import ba7_reference as R

SCENES = ["a", "b", "c"]


def _global_names(code):
    """the global names a code object and the functions nested in it load"""
    import dis
    names = {i.argval for i in dis.get_instructions(code) if i.opname == "LOAD_GLOBAL"}
    for c in code.co_consts:
        if hasattr(c, "co_code"):
            names |= _global_names(c)
    return names


def test_the_loop_and_the_projection_are_ba6_references_text():
    """...and every global name that text uses is one this module defines on purpose (the list in _over_this_layout's docstring)"""
    import builtins
    listed = {}
    for line in R._over_this_layout.__doc__.split("there and not silently):")[1].splitlines():
        words = line.split()
        if words and words[0] in ("lm_solve", "project_step", "quad_form", "jacobi_scale", "pcg_residual_and_floor"):
            cur = words[0]
            listed[cur] = set(words[1:])
        elif words:
            listed[cur] |= set(words)
    for name in ("lm_solve", "project_step", "quad_form", "jacobi_scale", "pcg_residual_and_floor"):
        f, g = getattr(R, name), getattr(R6, name)
        assert f.__code__ is g.__code__ and f.__globals__ is vars(R) and f is not g
        used = {n for n in _global_names(f.__code__) if not hasattr(builtins, n)}
        assert used == listed[name], (name, sorted(used ^ listed[name]))
        assert all(hasattr(R, n) for n in used)


@pytest.mark.parametrize("sname", ["a", "c"])
def test_focal_jacobian_against_central_differences_of_the_hp_residual(sname):
    sc = R.scene(sname)
    x = R.near_start(sname)
    _, Jp, Jrf = R.observe_np(sc, x)
    N = len(sc["cam_est"])
    h = 2.0 ** -10   # (r is linear in f: the difference quotient has no truncation error, only the rounding of the long double residual over h)
    worst = 0.0
    for k in ([0, 1, 2, 3, 4] if sname == "c" else [0, 7]):
        es = np.flatnonzero(sc["used"] & (sc["obs_cam"] == k))[:3]
        xp, xm = x.copy(), x.copy()
        xp[2 * N + k, 0] += h
        xm[2 * N + k, 0] -= h
        d = (R.residual_hp(sc, xp)[es] - R.residual_hp(sc, xm)[es]) / R.LD(2 * h)
        worst = max(worst, float(np.abs(d - Jrf[es, :, 3]).max() / np.abs(Jrf[es, :, 3]).max()))
        # an orientation coordinate and a centre coordinate through this module's layout
        for node, J in ((k, Jrf[:, :, :3]), (N + k, -Jp)):
            xp, xm = x.copy(), x.copy()
            xp[node, 1] += 2.0 ** -20
            xm[node, 1] -= 2.0 ** -20
            d = (R.residual_hp(sc, xp)[es] - R.residual_hp(sc, xm)[es]) / R.LD(2.0 ** -19)
            worst = max(worst, float(np.abs(d - J[es, :, 1]).max() / np.abs(J[es]).max()))
    print(sname, "central differences: worst relative deviation %.2e" % worst)
    assert worst <= 1e-9
    # the hp tier's own J_f: the same quotient to the rounding of a long double residual of a thousand pixels over 2 h
    Jf_hp = R.observe_hp(sc, x)[2][:, :, 3]
    es = np.flatnonzero(sc["used"] & (sc["obs_cam"] == 0))[:3]
    xp, xm = x.copy(), x.copy()
    xp[2 * N, 0] += h
    xm[2 * N, 0] -= h
    d = (R.residual_hp(sc, xp)[es] - R.residual_hp(sc, xm)[es]) / R.LD(2 * h)
    assert float(np.abs(d - Jf_hp[es]).max()) <= 64 * float(np.finfo(R.LD).eps) * 2e3 / (2 * h)


@pytest.mark.parametrize("sname", SCENES)
def test_all_seven_gauge_directions_are_null_vectors_of_the_jacobian_and_leave_the_focal_lengths(sname):
    sc = R.scene(sname)
    N = len(sc["cam_est"])
    x = R.near_start(sname)
    lin, _ = R.point_linearisation(sname, "huber", 10.0, False)
    scale = np.abs(lin["Jc"][:, :, :6]).max()
    dirs = R.gauge_directions(sc, x)
    assert len(dirs) == 7
    for i, v in enumerate(dirs):
        assert np.all(v[2 * N:3 * N] == 0)
        jv = np.abs(R.apply_J(sc, lin, v)).max()
        assert jv <= 1e-9 * scale * np.abs(v).max(), (i, jv, scale)
    # the focal direction is no gauge freedom: J does not annihilate it
    v = np.zeros_like(x)
    v[2 * N:3 * N, 0] = R.focal_of(sc, x)
    assert np.abs(R.apply_J(sc, lin, v)).max() > 1.0


@pytest.mark.parametrize("radius", [1e4, 1e10])
def test_reduced_solve_equals_the_full_solve_and_the_projection_keeps_the_model(radius):
    sc = R.scene("a")
    x = R.near_start("a")
    lin, asm = R.point_linearisation("a", "huber", 10.0, False)
    S = R.jacobi_scale(asm)
    y_full, dm = R.solve_step(sc, lin, asm, S, radius)
    Sc, rhs, _ = R.schur_system(sc, dm)
    yc = np.linalg.solve(Sc, rhs)
    y_red = np.concatenate([R.cam_nodes(yc), R.back_substitute(sc, dm, yc)])
    if radius == 1e4:
        assert np.abs(y_red - y_full).max() <= 1e-6 * np.abs(y_full).max()
    jd = [R.apply_J(sc, lin, np.where(dm["act"][:, None], -S * y, 0)) for y in (y_red, y_full)]
    assert np.abs(jd[0] - jd[1]).max() <= 1e-6 * np.abs(jd[1]).max()
    models = []
    for gauge in (True, False):
        d = R.project_step(sc, dm, y_full, x, gauge)
        models.append(-(d * asm["g"]).sum() - R.quad_form(sc, lin, d) / 2)
    assert abs(models[0] - models[1]) <= 1e-9 * abs(models[1])   # the projection leaves the model cost change unchanged
    d = R.project_step(sc, dm, y_full, x, True)
    for v in R.gauge_directions(sc, x):
        assert abs((d * v).sum()) <= 1e-10 * np.sqrt((d * d).sum() * (v * v).sum())


@pytest.mark.parametrize("sname", ["a", "c"])
def test_with_every_focal_length_held_the_system_and_the_step_are_ba6_references(sname):
    """The same numbers: ba6_reference at the generator's focal lengths against this module with focal_free = 0, from ba6_reference's near start"""
    s6 = R6.scene(sname)
    N = len(s6["cam_est"])
    sc = R.scene(sname, np.zeros(N, bool))
    x6 = R6.near_start(sname)
    x = R.nodes(x6[:N], x6[N:2 * N], s6["intrinsics"][:, 0], x6[2 * N:])
    lin6 = R6.linearise(*R6.observe_np(s6, x6), "huber", 10.0)
    asm6 = R6.assemble(s6, lin6)
    lin = R.linearise(*R.observe_np(sc, x), "huber", 10.0)
    asm = R.assemble(sc, lin)
    assert np.array_equal(asm["B"][:, :6, :6], asm6["B"]) and np.all(asm["B"][:, 6] == 0) and np.all(asm["B"][:, :, 6] == 0)
    assert np.array_equal(asm["g"][:2 * N], asm6["g"][:2 * N]) and np.array_equal(asm["g"][3 * N:], asm6["g"][2 * N:]) and np.all(asm["g"][2 * N:3 * N] == 0)
    for radius in (1e4, 1e10):
        y6, dm6 = R6.solve_step(s6, lin6, asm6, R6.jacobi_scale(asm6), radius)
        y, dm = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), radius)
        assert np.array_equal(dm["Bt"][:, :6, :6], dm6["Bt"]) and np.array_equal(dm["E"][:, :6], dm6["E"]) and np.all(dm["E"][:, 6] == 0)
        assert np.array_equal(dm["Ct"], dm6["Ct"]) and np.array_equal(dm["b7"][:, :6], dm6["b6"]) and np.all(dm["b7"][:, 6] == 0)
        Sc, rhs, _ = R.schur_system(sc, dm)
        Sc6, rhs6, _ = R6.schur_system(s6, dm6)
        keep = np.arange(7 * N) % 7 != 6
        assert np.array_equal(Sc[np.ix_(keep, keep)], Sc6) and np.array_equal(rhs[keep], rhs6)
        assert np.array_equal(Sc[~keep][:, ~keep], np.eye(N)) and np.all(Sc[np.ix_(~keep, keep)] == 0)
        # the full systems differ only by identity rows in other places: the solves agree to the rounding of the elimination order
        d6, d = R6.project_step(s6, dm6, y6, x6), R.project_step(sc, dm, y, x)
        assert np.all(d[2 * N:3 * N] == 0)
        jd6, jd = R6.apply_J(s6, lin6, d6), R.apply_J(sc, lin, d)
        assert np.abs(jd - jd6).max() <= 1e-9 * np.abs(jd6).max()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_conditions_on_the_cases_of_the_gpu_tests(name):
    """Both tiers take the same LM decisions, and no comparison lies within 1e-6 (relative) of its threshold: a condition on the inputs
    (the seeds and focal perturbations of ba7_reference.CASES were chosen for it), not a tolerance."""
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    sc = R.scene(R.CASES[name][0])
    f0, f1 = R.focal_of(sc, R.case_start(name)), R.focal_of(sc, hi["x"])
    print(name, R.TERM_NAMES[hi["termination"]], hi["iterations"], hi["successful"], hi["unsuccessful"], "cost %.6e -> %.6e" % (hi["initial_cost"], hi["final_cost"]),
          "margin %.2e" % R.decision_margin(hi["decisions"]))
    assert (lo["termination"], lo["iterations"], lo["successful"], lo["unsuccessful"]) == (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert [d[0] for d in lo["decisions"]] == [d[0] for d in hi["decisions"]]
    assert hi["termination"] in (0, 1, 2)
    assert R.decision_margin(hi["decisions"]) > 1e-6 and R.decision_margin(lo["decisions"]) > 1e-6
    assert hi["final_cost"] < hi["initial_cost"]
    act = sc["cam_active"]
    # the focal lengths start off and move (under Tukey a camera with every observation beyond the cut keeps its own: most move)
    assert np.all(f0[act] != sc["intrinsics"][act, 0]) and (f1[act] != f0[act]).sum() > act.sum() // 2 and np.array_equal(f1[~act], f0[~act])


def test_a_far_case_takes_a_rejected_step():
    far = [n for n in R.CASES if n.endswith("far")]
    assert len(far) == 4 and any(R.case_solve(n, True)["unsuccessful"] >= 1 for n in far)


@pytest.mark.parametrize("sname", ["a0", "b0", "c0"])
def test_noise_free_scenes_bring_the_hp_tiers_cost_to_the_stopping_rules_level(sname):
    """tests/test_gpu_ba7.py's test of the noise-free scenes says why no bound on the recovered scene is derived: |x| is dominated by the
    focal lengths, and what a last step of parameter_tolerance |x| leaves depends on the scene's conditioning.  What is asserted is what
    the stopping rules give (the minimum is 0: at most function_tolerance of the initial cost is left); the recovery is printed."""
    sc = R.scene(sname)
    out = R.lm_solve(sc, R.near_start(sname), hp=True)
    gen = R.nodes(sc["rot_aa"], sc["cam_pos"], sc["intrinsics"][:, 0], sc["gt_points"])
    err = np.abs(R.aligned(sc, out["x"], gen) - R.aligned(sc, gen, gen))
    nf = int(sc["cam_active"].sum())
    print(sname, R.TERM_NAMES[out["termination"]], out["iterations"], "cost %.3e -> %.3e" % (out["initial_cost"], out["final_cost"]), "scene error %.3e" % err[:-nf].max(),
          "focal error %.3e px" % err[-nf:].max())
    assert out["termination"] in (0, 1, 2) and out["final_cost"] <= 1e-6 * out["initial_cost"]


@pytest.mark.parametrize("hp", [False, True])
def test_scene_t_conditions_under_tukey(hp):
    """What tests/test_gpu_ba7.py asserts as exact zeros holds on the reference's own lin / asm at the near start: camera T_CAMERA's 7 x 7 block
    and gradient and track T_TRACK's are zero, and with the perturbed focal lengths every one of their observations is still beyond the cut."""
    sc = R.scene("t")
    N = len(sc["cam_est"])
    lin, asm = R.point_linearisation("t", *B.TUKEY, hp)
    tp = sc["track_ptr"].astype(np.int64)
    rows = np.concatenate([np.flatnonzero(sc["obs_cam"] == B.T_CAMERA), np.arange(tp[B.T_TRACK], tp[B.T_TRACK + 1])])
    assert np.all(lin["s"][rows] > 100.0)
    assert np.all(asm["B"][B.T_CAMERA] == 0) and np.all(asm["C"][B.T_TRACK] == 0)
    for node in (B.T_CAMERA, N + B.T_CAMERA, 2 * N + B.T_CAMERA, 3 * N + B.T_TRACK):
        assert np.all(asm["g"][node] == 0)
    for t, k, norm in B.T_AT_CUT:   # the observations placed at the cut are where they were put
        assert abs(float(np.sqrt(lin["s"][tp[t] + k])) - norm) <= 1e-6


@pytest.mark.parametrize("radius", [1e4, 1e10])
def test_scene_t_under_tukey_is_within_reach_of_the_pcg(radius):
    """A condition on the near start, not a reference: a float64 block-Jacobi PCG on the reference's own reduced system of scene t under
    Tukey reaches 1e-14 within max_cg_iterations (2000).  At radius 1e10 (more than half of the observations beyond the cut, blocks held up
    by a damping of 1e-16) that takes some 800 iterations with runs of more than a hundred without a quartering of r.M^-1 r, the longest of
    which is printed: gsfm_ba6's rule of 200 sits inside their range, which is why gsfm_ba7_options_default looks over half of the iteration
    budget (include/gsfm_ba7.h)."""
    sc = R.scene("t")
    lin, asm = R.point_linearisation("t", *B.TUKEY, True)
    its, longest = R.pcg_emulation(sc, R.damped(sc, lin, asm, R.jacobi_scale(asm), radius))
    print("radius %.0e: %s iterations, longest run without a mark %d" % (radius, its, longest))
    assert its is not None
    if radius == 1e4:
        assert longest < 100
