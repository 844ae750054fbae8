"""The reference system of one rotation LM step (tests/hp_reference.py: damped_system, step_residual, model_cost_change, the graphs of
tests/test_gpu_hp_step.py) checked on the CPU -- no GPU needed.

1. On a 12-camera graph the long-double helpers against a 40-digit mpmath solve of the same system.
2. For every case the device tests linearise at: the reference's own rounding floor at the exact solution is at most tol / 2 = 5e-13
   (a case that cannot meet it says nothing at cg_relative_tolerance = 1e-12), and the refined solve the tests compare with has a true
   residual far below that floor.  The floors are printed (pytest -s)."""
import mpmath
import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth

import hp_reference as H

LD = H.LD


def _mpf(x):
    return mpmath.mpf(np.format_float_positional(x, unique=False, precision=30, trim="-")) if x != 0 else mpmath.mpf(0)


def test_step_helpers_against_mpmath():
    g = synth.make_graph(12, 30, seed=5, outlier_frac=0.1)
    n, ei, ej = 12, g["edge_i"], g["edge_j"]
    ref = H.edge_set(_abi.ANGLE_AXIS, ei, ej, g["rel_aa"], g["init_aa"])
    lin = H.corrected(ref, "huber", (0.5,))
    A = H.assemble(lin, n, ei, ej)
    radius = 1e4
    sysm = H.damped_system(A, radius)
    K = H.system_matrix(lin, sysm, n, ei, ej)
    eps = float(np.finfo(LD).eps)
    with mpmath.workdps(40):
        # lam* from the diagonal of D*, in mpmath
        for k in range(n):
            for c in range(3):
                dd = _mpf(A["D"][k, c, c])
                sc = 1 / (1 + mpmath.sqrt(dd))
                lam = min(max(sc * sc * dd, mpmath.mpf("1e-6")), mpmath.mpf("1e32")) / (radius * sc * sc)
                assert abs(_mpf(sysm["lam"][k, c]) - lam) <= 8 * eps * lam
        Km = mpmath.matrix(3 * n, 3 * n)
        for r in range(3 * n):
            for c in range(3 * n):
                Km[r, c] = _mpf(K[r, c])
        bm = mpmath.matrix([_mpf(x) for x in sysm["b"].reshape(-1)])
        xm = mpmath.lu_solve(Km, bm)
        x = H.solve_refined(K, sysm["b"])
        xn = max(abs(v) for v in xm)
        assert max(abs(_mpf(x[k]) - xm[k]) for k in range(3 * n)) <= 1e3 * eps * xn
        gm = mpmath.matrix([_mpf(v) for v in A["g"].reshape(-1)])
        Hm = Km.copy()
        for k in range(3 * n):
            Hm[k, k] -= _mpf(sysm["lam"].reshape(-1)[k])
        mcc_mp = -(xm.T * gm)[0] - (xm.T * Hm * xm)[0] / 2
        # ||b||_{M^-1} in mpmath from the 3 x 3 blocks of K
        bn2 = mpmath.mpf(0)
        for k in range(n):
            Mk = Km[3 * k:3 * k + 3, 3 * k:3 * k + 3]
            bk = bm[3 * k:3 * k + 3]
            bn2 += (bk.T * mpmath.lu_solve(Mk, bk))[0]
        assert abs(_mpf(H.mnorm(sysm, sysm["b"])) - mpmath.sqrt(bn2)) <= 1e3 * eps * mpmath.sqrt(bn2)
    xs = x.reshape(n, 3)
    mcc, mag = H.model_cost_change(lin, A, n, ei, ej, xs)
    assert mcc > 0
    assert abs(_mpf(mcc) - mcc_mp) <= 1e3 * eps * float(mag)
    rel, floor, _ = H.step_residual(lin, A, sysm, n, ei, ej, xs)
    print("12 cameras: residual of the refined solve %.2e, floor %.2e" % (rel, floor))
    assert rel <= 1e-17 and 0 < floor <= H.STEP_FLOOR_MAX
    # the check sees a step that is off by one part in 1e9, and one camera's step alone
    rel_bad, _, _ = H.step_residual(lin, A, sysm, n, ei, ej, xs * (1 + LD(1e-9)))
    assert 0.5e-9 <= rel_bad <= 2e-9, rel_bad
    one = xs.copy()
    one[7] *= 1 + LD(1e-9)
    assert H.step_residual(lin, A, sysm, n, ei, ej, one)[0] > 100 * floor
    # per-component norms: restricting to all cameras is the whole norm
    assert H.step_residual(lin, A, sysm, n, ei, ej, xs, cams=np.arange(n))[1] == floor


@pytest.mark.parametrize("case", H.STEP_CASES, ids=lambda c: "%s-et%d-%s-r%.0e" % c)
def test_reference_floor_at_the_exact_solution(case):
    name, et, lname, radius = case
    g, lin, A, sysm = H.step_reference(name, et, lname, radius)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    xs = H.step_solution(name, et, lname, radius)
    rel, floor, _ = H.step_residual(lin, A, sysm, n, ei, ej, xs)
    step = np.sqrt((xs.astype(float) ** 2).sum(axis=1))
    print("%s et %d %s radius %.0e: %d cameras %d edges, floor %.2e, residual of the refined solve %.1e, step rms %.2e max %.2e rad"
          % (name, et, lname, radius, n, len(ei), floor, rel, float(np.sqrt((step ** 2).mean())), float(step.max())))
    assert floor <= H.STEP_FLOOR_MAX, floor
    assert rel <= 1e-3 * floor, rel
    if et == _abi.QUATERNION_NORM:   # no edge at the sign canonicalisation's discontinuity
        q = synth.aa_to_quat(g["rot"])
        est = synth.quat_mul(synth.aa_to_quat(g["rel_aa"]), q[g["edge_i"]])
        assert np.abs(est[:, 1]).min() > 1e-9 and np.abs(q[:, 1]).min() > 1e-9
    if name == "twocomp":
        for c in (0, 1):
            cams = np.flatnonzero(g["comp"] == c)
            rc, fc, _ = H.step_residual(lin, A, sysm, n, ei, ej, xs, cams=cams)
            print("   component %d (%d cameras): floor %.2e residual %.1e" % (c, len(cams), fc, rc))
            assert fc <= H.STEP_FLOOR_MAX
        assert np.all(xs[g["comp"] == 2] == 0) and np.all(A["deg"][g["comp"] == 2] == 0)
