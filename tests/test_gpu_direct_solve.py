"""-m gpu: the DEVICE's Levenberg-Marquardt step above the dense-Cholesky sizes against a direct solve of the normal equations.

The reference solves every graph with SPARSE_NORMAL_CHOLESKY (/root/reference/src/GSfM_nonlinear_rotation_estimator.cpp:299-305); the
device uses block-Jacobi PCG beyond 512 cameras.  For three consecutive LM iterations (each restarted from the previous device iterate, so
both sides linearise at bit-identical rotations) the device's accepted step must equal x (+) (-scale * y) with y from a DIRECT factorisation
(scipy / LAPACK) of the oracle's damped normal equations at that point: to 1e-10 of the step with PCG run to 1e-14 (the oracle's own
setting), and to 1e-8 of the step at the product's default relative residual of 1e-12 (the systems are weakly damped: the step error is the
residual times a condition number of 1e3-1e4; in absolute terms 3e-12 rad here, against the parity bar of 1e-6).  The oracle's own PCG
is held to the same direct solves in tests/test_oracle_direct_solve.py (CPU).  Up to 5 333 cameras the device can also take the step exactly
(dense_cholesky_max_cams): that step is held to the same direct solve, the Trafalgar-sized case (5 288 cameras, 3N = 15 864) included."""
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem
from test_oracle_direct_solve import direct_step

pytestmark = pytest.mark.gpu

CASES = [   # name, cameras, edges, error type, loss, outliers, local window, sparse LU, environment
    ("random 2000/40k covariance + MAGSAC", 2000, 40000, _abi.ANGLE_AXIS_COVARIANCE, lambda: LF.MAGSACWeightBasedLoss(0.02), 0.3, 0, False, {}),
    ("random 2000/40k SoftL1, column-sorted kernels", 2000, 40000, _abi.ANGLE_AXIS, lambda: LF.SoftLOneLoss(0.1), 0.3, 0, False, {"GSFM_K3_COLSORT": "1"}),
    ("Trafalgar-sized random 5288/80k covariance + MAGSAC", 5288, 80000, _abi.ANGLE_AXIS_COVARIANCE, lambda: LF.MAGSACWeightBasedLoss(0.02), 0.3, 0, False, {}),
    ("Trafalgar-sized and Trafalgar-dense random 5288/680k covariance + MAGSAC (column-sorted layout chosen by the density rule)", 5288, 680000, _abi.ANGLE_AXIS_COVARIANCE, lambda: LF.MAGSACWeightBasedLoss(0.02), 0.3, 0, False, {}),
    ("C2-sized coherent 10k/200k Geman-McClure", 10000, 200000, _abi.ANGLE_AXIS, lambda: LF.GemanMcClureLoss(0.1, 1.0), 0.1, 120, True, {}),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_lm_step_equals_a_direct_solve(oracle, case):
    name, n, e, et, mk, outl, window, sparse, env = CASES[case]
    g = synth.make_graph(n, e, 11, outlier_frac=outl, local_window=window)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev = RotationProblem(n, g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    dev.set_loss(mk())
    if e == 680000:
        assert dev.matvec_bytes()[1] == 2   # 1.36 M directed entries without locality: K2c / K3c, and the dense assembly from that layout
    o = oracle.OracleProblem(n, g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"])
    o.set_loss(mk())
    o.set_linear_solver("pcg")
    x = g["init_aa"].copy()
    for k in range(3):
        o.capture_steps(1)
        o.solve(x, max_num_iterations=1)
        sysk = o.captured_step(0)
        y, _ = direct_step(sysk, g["edge_i"], g["edge_j"], n, sparse)
        delta = (-y * sysk["scale"]).reshape(n, 3)
        rt, st = dev.solve(x, max_num_iterations=1, cg_relative_tolerance=1e-14)
        rd, sd = dev.solve(x, max_num_iterations=1)
        for s_ in (sd, st):
            assert s_["num_successful_steps"] == 1 and s_["num_dense_solves"] == 0 and s_["num_cg_iterations"] > 0, s_
        err, err_t, dmax = np.abs(rd - (x + delta)).max(), np.abs(rt - (x + delta)).max(), np.abs(delta).max()
        print("%s, step %d from the device's own iterate: |delta|_inf = %.2e; |x_dev - (x + delta_direct)|_inf = %.2e with PCG to 1e-12 (%d iterations), %.2e with PCG to 1e-14 (%d)" % (
            name, k + 1, dmax, err, sd["num_cg_iterations"], err_t, st["num_cg_iterations"]))
        # (round 5: no solve runs below the absolute floor of the step -- block-Jacobi's estimate of what any camera still lacks under 2e-14 rad,
        # cam_kernels.hpp k_cam_bound; the true error is that times the conditioning the docstring speaks of: a few 1e-12 rad at most)
        assert err_t <= max(1e-10 * dmax, 5e-12), (name, k, err_t)
        assert err <= max(1e-8 * dmax, 5e-12), (name, k, err)
        if n <= 5333 and not env:
            # the device's own exact step at this size (tiled Cholesky, trailing update on the fp64 matrix cores) against the same direct solve
            rx, sx = dev.solve(x, max_num_iterations=1, dense_cholesky_max_cams=n)
            assert sx["num_dense_solves"] == 1 and sx["num_cg_iterations"] == 0 and sx["num_successful_steps"] == 1, sx
            err_x = np.abs(rx - (x + delta)).max()
            print("    device dense Cholesky step: |x_dev - (x + delta_direct)|_inf = %.2e" % err_x)
            assert err_x <= 1e-10 * dmax, (name, k, err_x)
        x = rd
