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
    """J~^T r~ is the gradient of rho(|r|^2) / 2: rho' J^T r, for both Huber branches and SoftLOne."""
    sc = R.scene("a")
    c0, p0 = R.perturbed_start(sc, 0.05, 0.05, 1)
    r, J = R.observe_np(sc, c0, p0)
    for kind in ("huber", "softl1"):
        lin = R.linearise(r, J, kind, 10.0)
        _, rho1, _ = R.loss_rho(kind, 10.0, lin["s"])
        want = rho1[:, None] * np.einsum("eki,ek->ei", J, r)
        assert np.abs(lin["a"] - want).max() <= 1e-12 * np.abs(want).max()
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
