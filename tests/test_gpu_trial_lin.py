"""The fused trial evaluation (csrc/colsort_kernels.hpp, K2c with the cost; csrc/solver_lm.hpp, evaluate_trial): on the column-sorted layout a
trial point the LM loop expects to accept is linearised into a spare set of blocks while its cost is taken, instead of a K1 sweep now and a
linearisation after the acceptance.  Its blocks, g and D must be launch_lin's bit for bit, its cost K1's to rounding, a trial that is not
accepted must leave the current linearisation alone, and the solve must take the same LM path with GSFM_TRIAL_LIN=0 or 1."""
import ctypes as C
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem

pytestmark = pytest.mark.gpu

_DP = C.POINTER(C.c_double)


class _Env:
    def __init__(self, **kw): self.kw = {k: str(v) for k, v in kw.items()}
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def _check_fn():
    f = _abi.load_library().gsfm_rot_trial_lin_check
    f.argtypes = [C.c_void_p, _DP, _DP, _DP, C.POINTER(C.c_int32)]
    f.restype = C.c_int
    return f


def _trial_lin_check(p, rot, rot_trial):
    rot = np.ascontiguousarray(rot, dtype=np.float64)
    rot_trial = np.ascontiguousarray(rot_trial, dtype=np.float64)
    cost = np.zeros(2)
    same = (C.c_int32 * 2)()
    st = _check_fn()(p._h, rot.ctypes.data_as(_DP), rot_trial.ctypes.data_as(_DP), cost.ctypes.data_as(_DP), same)
    return st, cost, [int(same[0]), int(same[1])]


def _problem(g, et, colsort=None, **env):
    kw = dict(env)
    if colsort is not None: kw["GSFM_K3_COLSORT"] = colsort
    if et == _abi.ANGLE_AXIS_COVARIANCE: kw["GSFM_QREL3"] = 1   # (the three-component planes, W_MATRIX3: what C5 runs)
    with _Env(**kw):
        return RotationProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"], inlier_weight=g["inlier_weight"])


@pytest.mark.parametrize("et", [_abi.ANGLE_AXIS_COVTRACE, _abi.ANGLE_AXIS_COVARIANCE])
@pytest.mark.parametrize("shape", ["small", "c5_degree"])
def test_fused_trial_blocks_are_launch_lins_and_its_cost_is_k1s(et, shape):
    """Scalar (W = 1) and three-component covariance (W = 3) whitening, the MAGSAC nu = 3 and a Huber loss; a small graph forced onto the
    column-sorted layout and one of C5's degree (200 edges per camera) that takes it by itself.  The trial point is 3 degrees away from the
    linearisation point."""
    n, m = (1500, 30000) if shape == "small" else (20000, 2000000)
    g = synth.make_graph(n, m, seed=91, outlier_frac=0.3)
    p = _problem(g, et, colsort=1 if shape == "small" else None)
    assert int(p.matvec_bytes()[1]) == 2   # column-sorted
    rng = np.random.default_rng(5)
    trial = g["init_aa"] + np.deg2rad(3.0) / np.sqrt(3.0) * rng.standard_normal(g["init_aa"].shape)
    for loss in (LF.MAGSACWeightBasedLoss(0.02), LF.HuberLoss(0.05)):
        p.set_loss(loss)
        st, cost, same = _trial_lin_check(p, g["init_aa"], trial)
        print("%s %s %s: K1 %.17g fused %.17g (rel %.2e), blocks same %d, current untouched %d"
              % (shape, et, type(loss).__name__, cost[0], cost[1], abs(cost[1] - cost[0]) / cost[0], same[0], same[1]))
        assert st == 0, st
        assert same == [1, 1]
        assert cost[0] > 0 and abs(cost[1] - cost[0]) <= 1e-13 * cost[0]
    p.close()


def test_solves_with_and_without_the_fused_trial_take_the_same_path():
    """GSFM_TRIAL_LIN=0 restores K1 at every trial point; the LM path (iterations, terminations, step counts, the counters of the evaluations
    Ceres counts) is the same, the rotations agree to 1e-12 rad and the costs to 1e-12 relative.  Both forcing schedules."""
    g = synth.make_graph(20000, 2000000, seed=2023, outlier_frac=0.3)
    p = _problem(g, _abi.ANGLE_AXIS_COVARIANCE)
    p.set_loss(LF.MAGSACWeightBasedLoss(0.02))
    assert _trial_lin_check(p, g["init_aa"], g["init_aa"])[0] == 0   # the problem has the fused evaluation
    keys = ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_residual_sweeps", "num_linearizations")
    for forcing in (1, 0):
        out = {}
        for on in (0, 1):
            with _Env(GSFM_TRIAL_LIN=on):
                r, s = p.solve(g["init_aa"], pcg_forcing=forcing)
            out[on] = (r, s)
        (r0, s0), (r1, s1) = out[0], out[1]
        print("forcing %d: off %s / on %s" % (forcing, [s0[k] for k in keys], [s1[k] for k in keys]))
        for k in keys:
            assert s0[k] == s1[k], k
        assert abs(s1["final_cost"] - s0["final_cost"]) <= 1e-12 * s0["final_cost"]
        assert abs(s1["initial_cost"] - s0["initial_cost"]) <= 1e-12 * s0["initial_cost"]
        assert synth.angular_distance(r1, r0).max() <= 1e-12
    p.close()


def test_without_room_for_the_spare_set_the_solve_is_todays():
    """The spare set is allocated only if it leaves GSFM_TRIAL_LIN_RESERVE_MB free; forced not to fit, the problem has no fused evaluation and
    its solve gives the bits of GSFM_TRIAL_LIN=0 on a problem that has one."""
    g = synth.make_graph(1500, 30000, seed=17, outlier_frac=0.3)
    full = _problem(g, _abi.ANGLE_AXIS_COVARIANCE, colsort=1)
    tight = _problem(g, _abi.ANGLE_AXIS_COVARIANCE, colsort=1, GSFM_TRIAL_LIN_RESERVE_MB=1e12)
    for p in (full, tight):
        p.set_loss(LF.MAGSACWeightBasedLoss(0.02))
    assert _trial_lin_check(full, g["init_aa"], g["init_aa"])[0] == 0
    assert _trial_lin_check(tight, g["init_aa"], g["init_aa"])[0] == 6   # GSFM_ERR_UNSUPPORTED
    with _Env(GSFM_TRIAL_LIN=0):
        r0, s0 = full.solve(g["init_aa"])
    r1, s1 = tight.solve(g["init_aa"])
    assert np.array_equal(r0, r1)
    assert s0["final_cost"] == s1["final_cost"] and s0["num_iterations"] == s1["num_iterations"] and s0["num_cg_iterations"] == s1["num_cg_iterations"]
    full.close(); tight.close()
