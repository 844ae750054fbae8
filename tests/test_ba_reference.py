"""CPU checks of the bundle-adjustment reference (tests/ba_reference.py) and of the conditions the GPU tests (tests/test_gpu_ba.py) rely
on, asserted here on the reference alone so that a device run cannot legitimately differ."""
import mpmath
import numpy as np
import pytest

import ba_reference as R


def test_jacobian_against_central_differences():
    """The closed-form point Jacobian in mpmath against central differences of the mpmath residual (h = 1e-14: truncation ~ h^2), the camera
    Jacobian being its negative (the residual depends on X - o alone); and the fp64 tier's J against it."""
    sc = R.scene("a")
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    _, Jnp = R.observe_np(sc, c0, p0)
    with mpmath.workdps(R.MP_DPS):
        h = mpmath.mpf("1e-14")
        for e in np.flatnonzero(sc["used"])[::7]:
            c, t = int(sc["obs_cam"][e]), int(sc["track_of"][e])
            Rm = R.rotation_mp(sc["rot_aa"][c])
            K = [R._mp(x) for x in sc["intrinsics"][c]]
            xy = [R._mp(x) for x in sc["obs_xy"][e]]
            X, o = [R._mp(x) for x in p0[t]], [R._mp(x) for x in c0[c]]
            _, p = R.residual_mp(Rm, K, xy, X, o)
            J = R.jacobian_mp(Rm, K, p)
            scale = max(abs(v) for row in J for v in row)
            for j in range(3):
                Xp, Xm, op, om = list(X), list(X), list(o), list(o)
                Xp[j] += h; Xm[j] -= h; op[j] += h; om[j] -= h
                for i in range(2):
                    d_point = (R.residual_mp(Rm, K, xy, Xp, o)[0][i] - R.residual_mp(Rm, K, xy, Xm, o)[0][i]) / (2 * h)
                    d_cam = (R.residual_mp(Rm, K, xy, X, op)[0][i] - R.residual_mp(Rm, K, xy, X, om)[0][i]) / (2 * h)
                    assert abs(d_point - J[i][j]) <= mpmath.mpf("1e-20") * scale
                    assert abs(d_cam + J[i][j]) <= mpmath.mpf("1e-20") * scale
                    assert abs(R._mp(Jnp[e, i, j]) - J[i][j]) <= mpmath.mpf("1e-12") * scale


def test_corrector_matches_the_robustified_cost():
    """J~^T r~ is the gradient of rho(|r|^2) / 2: rho' J^T r, for both Huber branches, SoftLOne, both Tukey branches and Geman-McClure."""
    sc = R.scene("a")
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    r, J = R.observe_np(sc, c0, p0)
    for kind, a in (("huber", 10.0), ("softl1", 10.0), R.TUKEY, R.GEMAN):
        with np.errstate(all="raise"):   # (finite where used: nothing the reference keeps divides by rho' = 0)
            lin = R.linearise(r, J, kind, a)
        _, rho1, _ = R.loss_rho(kind, a, lin["s"])
        want = rho1[:, None] * np.einsum("eki,ek->ei", J, r)
        assert np.abs(lin["a"] - want).max() <= 1e-12 * np.abs(want).max()
        assert all(np.all(np.isfinite(lin[k])) for k in ("rho", "H", "a", "rt", "Jt"))
    lin = R.linearise(r, J, *R.TUKEY)
    cut = lin["s"] > 100.0
    assert cut[sc["used"]].any() and (~cut[sc["used"]]).any()
    assert np.all(lin["Jt"][cut] == 0) and np.all(lin["rt"][cut] == 0) and np.all(lin["rho"][cut] == 100.0 / 6)
    s = R.linearise(r, J, "huber", 10.0)["s"][sc["used"]]
    assert (s > 100.0).any() and (s < 100.0).any()   # both branches occur at the point the GPU tests linearise at


def test_schur_identity_in_mpmath():
    """The reduced solve plus back-substitution equals the solve of the full damped system, both in mpmath on a 4-camera scene."""
    from globalsfmpy_amd import synth
    s = synth.make_tracks(4, 8, 3, lengths=(2, 3, 4), noise_px=0.5)
    sc = R._finish({k: s[k] for k in ("rot_aa", "cam_pos", "intrinsics", "track_ptr", "obs_cam", "obs_xy", "gt_points")}, None, None)
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    r, J = R.observe_hp(sc, c0, p0)
    lin = R.linearise(r, J, "huber", 10.0)
    asm = R.assemble(sc, lin)
    dm = R.damped(sc, lin, asm, R.jacobi_scale(asm), 1e4)
    K, b = R.full_system(sc, dm)
    Sc, rhs, _ = R.schur_system(sc, dm)
    N = 4
    with mpmath.workdps(R.MP_DPS):
        mp = lambda A: mpmath.matrix([[mpmath.mpf(str(v)) for v in row] for row in np.atleast_2d(A).tolist()])
        Km, bm = mp(K), mp(b).T
        y_full = mpmath.lu_solve(Km, bm)
        n, nc = Km.rows, 3 * N
        A, Eb, Cb = Km[:nc, :nc], Km[:nc, nc:], Km[nc:, nc:]
        Ci = Cb ** -1
        Sm = A - Eb * Ci * Eb.T
        rm = bm[:nc] - Eb * (Ci * bm[nc:])
        yc = mpmath.lu_solve(Sm, rm)
        yp = Ci * (bm[nc:] - Eb.T * yc)
        scale = max(abs(v) for v in y_full)
        worst = max([abs(yc[k] - y_full[k]) for k in range(nc)] + [abs(yp[k] - y_full[nc + k]) for k in range(n - nc)])
        assert worst <= mpmath.mpf("1e-25") * scale, worst / scale
        # the long-double tier's reduced system is that one
        s_scale, r_scale = max(abs(v) for v in Sm), max(abs(v) for v in rm)
        assert max(abs(mpmath.mpf(str(Sc[i, j])) - Sm[i, j]) for i in range(nc) for j in range(nc)) <= mpmath.mpf("1e-16") * s_scale
        assert max(abs(mpmath.mpf(str(rhs[i])) - rm[i]) for i in range(nc)) <= mpmath.mpf("1e-16") * r_scale
    # and the long-double tier's own reduced solve agrees with it
    y_ld, _ = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), 1e4, hp=True)
    assert max(abs(float(y_ld.reshape(-1)[k]) - float(y_full[k])) for k in range(len(b))) <= 1e-13 * float(scale)


@pytest.mark.parametrize("sname", ["a", "b"])
def test_gauge_directions_are_null_vectors_of_the_jacobian(sname):
    """J v = 0 for the three translations and for the scaling about the centroid of the active nodes (hp tier)."""
    sc = R.scene(sname)
    lin, _ = R.point_linearisation(sname, "huber", 10.0, True)
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    x = np.concatenate([c0, p0]).astype(R.LD)
    act = np.concatenate([sc["cam_active"], sc["pt_active"]])
    dirs = [np.where(act[:, None], np.eye(3, dtype=R.LD)[c][None, :], 0) for c in range(3)]
    dirs.append(np.where(act[:, None], x - x[act].mean(0), 0))
    jn = np.sqrt((lin["Jt"] ** 2).sum())
    for v in dirs:
        assert np.abs(R.apply_J(sc, lin, v)).max() <= 1e-15 * float(jn) * float(np.sqrt((v * v).sum()))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_conditions_on_the_scenes_of_the_gpu_tests(name):
    """Every solve ends on a tolerance, not on the iteration cap; the far starts take at least one rejected step; no accept / reject or
    termination comparison lies within 1e-6 (relative) of its threshold; the fp64 and the hp tier take the same decisions."""
    lo, hi = R.case_solve(name, False), R.case_solve(name, True)
    for o in (lo, hi):
        assert o["termination"] in (0, 1, 2), R.TERM_NAMES[o["termination"]]
        assert o["iterations"] < R.DEFAULTS["max_num_iterations"]
        assert R.decision_margin(o["decisions"]) > 1e-6
        if name.endswith("far"):
            assert o["unsuccessful"] >= 1
    assert (lo["termination"], lo["iterations"], lo["successful"], lo["unsuccessful"]) == (hi["termination"], hi["iterations"], hi["successful"], hi["unsuccessful"])
    assert [a for a, _ in lo["trace"]] == [a for a, _ in hi["trace"]]
    assert [n for n, _, _ in lo["decisions"]] == [n for n, _, _ in hi["decisions"]]


@pytest.mark.parametrize("sname", ["a0", "b0"])
def test_noise_free_scenes_end_on_a_tolerance_at_the_generator_scene(sname):
    sc = R.scene(sname)
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    o = R.lm_solve(sc, c0, p0)
    assert o["termination"] in (0, 1, 2) and R.decision_margin(o["decisions"]) > 1e-6
    assert np.abs(R.normalise(sc, o["cam"], o["points"]) - R.normalise(sc, sc["cam_pos"], sc["gt_points"])).max() <= 1e-6


# ---- Tukey and Geman-McClure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, R.LD])
def test_tukey_and_geman_mcclure_rows_against_the_loss_classes(dtype):
    """loss_rho against loss_functions.TukeyLoss / GemanMcClureLoss.Evaluate (pinned to the reference project's vectors by
    tests/test_oracle_golden.py) at s = 0, inside, at the cut, beyond: a few roundings of float64."""
    from globalsfmpy_amd import loss_functions as LF
    s = np.array([0.0, 1e-3, 37.0, 99.999, 100.0, 100.0 + 1e-9, 2500.0, 1e8])
    for (kind, a), cls, floor in ((R.TUKEY, LF.TukeyLoss(10.0), (100.0 / 6, 0.5, 0.01)), (R.GEMAN, LF.GemanMcClureLoss(10.0, 0.5), (0.0, 0.0, 0.0))):
        got = R.loss_rho(kind, a, s.astype(dtype))
        assert all(g.dtype == dtype for g in got)
        for i, si in enumerate(s):
            want = [0.0, 0.0, 0.0]
            cls.Evaluate(float(si), want)
            for k in range(3):
                assert abs(float(got[k][i]) - want[k]) <= 8 * R.U * max(abs(want[k]), floor[k]), (kind, si, k)
    t = R.loss_rho(*R.TUKEY, np.array([100.0, 100.0 + 1e-9], dtype))
    assert t[1][0] == 0 and t[1][1] == 0 and t[0][1] == dtype(100) / 6 and t[2][1] == 0


def _scene_t_conditions(mod, lin, asm):
    sc = mod.scene("t")
    tp = sc["track_ptr"].astype(np.int64)
    s = lin["s"]
    cam_rows = np.flatnonzero(sc["obs_cam"] == R.T_CAMERA)
    track_rows = np.arange(tp[R.T_TRACK], tp[R.T_TRACK + 1])
    assert len(cam_rows) == 3 and len(track_rows) == 2 and sc["used"].all()
    assert np.all(s[cam_rows] > 100.0) and np.all(s[track_rows] > 100.0)
    assert np.all(asm["B"][R.T_CAMERA] == 0) and np.all(asm["C"][R.T_TRACK] == 0)     # exactly
    others = np.setdiff1d(np.arange(len(s)), np.concatenate([cam_rows, track_rows]))
    assert (s[others] > 100.0).any() and (s[others] <= 100.0).any()                   # both branches among the rest
    for t, k in R.T_SINGLE:
        assert s[tp[t] + k] > 100.0
    n = np.sqrt(np.asarray(s, np.float64))
    assert ((n > 9.9) & (n <= 10.0)).any() and ((n > 10.0) & (n < 10.1)).any()        # within 1 % of the cut, on either side
    return cam_rows, track_rows


@pytest.mark.parametrize("hp", [False, True])
def test_scene_t_conditions_under_tukey(hp):
    """What the GPU tests assert as exact zeros holds on the reference's own lin / asm at the near start, in both tiers."""
    sc = R.scene("t")
    N = len(sc["cam_est"])
    lin, asm = R.point_linearisation("t", *R.TUKEY, hp)
    cam_rows, track_rows = _scene_t_conditions(R, lin, asm)
    assert np.all(asm["g"][R.T_CAMERA] == 0) and np.all(asm["g"][N + R.T_TRACK] == 0)
    assert np.all(lin["rho"][np.concatenate([cam_rows, track_rows])] == lin["rho"].dtype.type(100) / 6)
    for radius in (1e4, 1e10):
        y, dm = R.solve_step(sc, lin, asm, R.jacobi_scale(asm), radius, hp=hp)
        assert np.all(dm["S"][[R.T_CAMERA, N + R.T_TRACK]] == 1)
        d2 = dm["S"].dtype.type(R.DEFAULTS["min_lm_diagonal"]) / dm["S"].dtype.type(radius)
        assert np.all(dm["Bt"][R.T_CAMERA] == d2 * np.eye(3)) and np.all(dm["Ct"][R.T_TRACK] == d2 * np.eye(3))
        Sc = R.schur_system(sc, dm)[0]
        rows = slice(3 * R.T_CAMERA, 3 * R.T_CAMERA + 3)
        assert np.all(Sc[rows, rows] == d2 * np.eye(3)) and np.count_nonzero(Sc[rows]) == 3     # S reduces to the damping there
        plain = R.project_step(sc, dm, y, np.zeros_like(y), gauge=False)
        assert np.all(plain[[R.T_CAMERA, N + R.T_TRACK]] == 0)                                  # the plain step leaves both where they are


def test_cut_camera_and_track_of_scene_t_through_a_solve():
    """t_near_tukey: camera 4's and track 5's observations are beyond the cut at the end as at the start.  With the default gauge projection
    both move (it subtracts the mean step and the scale component from every active node); without it they keep their input bytes, since
    their step is exactly zero (zero gradient, zero coupling).  tests/test_gpu_ba.py asserts both of the device."""
    sc = R.scene("t")
    c0, p0 = R.case_start("t_near_tukey")
    for o, moved in ((R.case_solve("t_near_tukey", False), True), (R.lm_solve(sc, c0, p0, *R.TUKEY, remove_gauge=0), False)):
        lin = R.linearise(*R.observe_np(sc, o["cam"], o["points"]), *R.TUKEY)
        asm = R.assemble(sc, lin)
        assert np.all(asm["B"][R.T_CAMERA] == 0) and np.all(asm["C"][R.T_TRACK] == 0)
        assert o["termination"] in (0, 1, 2) and o["iterations"] >= 3
        assert (o["cam"][R.T_CAMERA].tobytes() != c0[R.T_CAMERA].tobytes()) == moved and (o["points"][R.T_TRACK].tobytes() != p0[R.T_TRACK].tobytes()) == moved


@pytest.mark.parametrize("name", sorted(R.DEFECTS))
def test_a_defective_loss_exceeds_the_bound_of_the_gpu_tests(name):
    """The bound the device is held to is tight enough to notice each defect: the fp64 tier WITH the defect, put where the device's output
    goes in the GPU test's ratio (scene a, near start), is above 1 on the gradient and on the blocks."""
    kind, a = R.DEFECTS[name]
    sc = R.scene("a")
    N = len(sc["cam_est"])
    lin64, asm64 = R.point_linearisation("a", kind, a, False)
    _, asmhp = R.point_linearisation("a", kind, a, True)
    with R.defect(name):
        bad = R.assemble(sc, R.linearise(*R.observe_np(sc, *R.perturbed_start(sc, 0.05, 0.05, 1)), kind, a))
    worst = {"g_cam": R.ratio(bad["g"][:N], asm64["g"][:N], asmhp["g"][:N]), "g_point": R.ratio(bad["g"][N:], asm64["g"][N:], asmhp["g"][N:]),
             "B": R.ratio(bad["B"], asm64["B"], asmhp["B"]), "C": R.ratio(bad["C"], asm64["C"], asmhp["C"])}
    print(name, worst)
    assert min(worst.values()) > 1.0
    assert R.ratio(asm64["g"], asm64["g"], asmhp["g"]) <= 1.0 / R.MARGIN     # (and the same arithmetic without the defect is inside it)


def test_hp_point_solve_against_mpmath_on_a_rank_two_block():
    """The hp tier's c_solve on the block that decided its form: one observation (T: 2 x 3, entries of order one) held up by a damping of
    1e-10, condition 1e10.  E~ C~^-1 E~^T is T C~^-1 T^T = I - (I + T D^-2 T^T)^-1 here: of order one, 1e-10 short of the identity.  Against a
    40-digit mpmath solve of the same long-double block c_solve keeps it to a few roundings of long double (2^-64 each, some thirty
    operations: 1e-17), so that what is left of I - T C~^-1 T^T, the point's whole contribution to the reduced matrix, has seven digits; the
    rounded explicit inverse the tier used before is wrong by 1e-19 / 1e-10 in every entry and loses all of them."""
    rng = np.random.default_rng(7)
    T = rng.standard_normal((2, 3)).astype(R.LD)
    d2 = R.LD(1e-10) * np.array([0.3, 0.5, 0.2], R.LD)
    Ct = T.T @ T + np.diag(d2)
    dm = {"Cchol": np.array([R._chol3(Ct)])}
    got = T @ R.c_solve(dm, 0, T.T.copy())
    to_mp = lambda x: mpmath.mpf(float(x)) + mpmath.mpf(float(x - R.LD(float(x))))     # a long double, exactly
    with mpmath.workdps(R.MP_DPS):
        Cm = mpmath.matrix([[to_mp(v) for v in row] for row in Ct])
        Tm = mpmath.matrix([[to_mp(v) for v in row] for row in T])
        want = Tm * (Cm ** -1) * Tm.T
        err = max(abs(to_mp(got[i, j]) - want[i, j]) for i in range(2) for j in range(2))
        rest = max(abs((1 if i == j else 0) - want[i, j]) for i in range(2) for j in range(2))
        old = T @ np.array([[R._ld(v) for v in row] for row in (Cm ** -1).tolist()], R.LD) @ T.T      # the 40-digit inverse, rounded, then multiplied
        err_old = max(abs(to_mp(old[i, j]) - want[i, j]) for i in range(2) for j in range(2))
    print("T C~^-1 T^T: c_solve off by %.2e, the rounded inverse by %.2e; I - T C~^-1 T^T is %.2e" % (float(err), float(err_old), float(rest)))
    assert 1e-11 < float(rest) < 1e-8
    assert float(err) <= 1e-17 and float(err_old) > 100 * float(err)
