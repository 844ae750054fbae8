"""CPU check of the host trust-region rule (csrc/trust_region.hpp, used by LmSolve and lm_loop.hpp): the host compiler builds
tests/cpp/trust_region_test.cpp against the header.  The program's own checks cover five consecutive invalid steps (the radius shrinks by
2, 4, 8, 16, the fifth ends the solve); the replay feeds it the steps of a CPU-oracle solve and wants the oracle's radius column bit for bit."""
import os
import subprocess

import numpy as np

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import loss_functions as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "trust_region_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "trust_region_test.cpp"), "-o", exe])
    return exe


def test_invalid_steps_and_resets(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr


def test_replay_of_an_oracle_trace_is_bit_identical(oracle, tmp_path):
    """A far start under a Cauchy loss: 54 LM iterations with rejected steps and accepted ones whose relative decrease is below 0.937, where
    the law radius / max(1/3, 1 - (2 rho - 1)^3) is not clamped at 3 x and every bit of std::pow shows.  The rows are classified as
    _replay_radius of test_gpu_round5.py classifies them."""
    g = synth.make_graph(40, 160, seed=1, outlier_frac=0.3)
    o = oracle.OracleProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], _abi.ANGLE_AXIS)
    o.set_loss(LF.CauchyLoss(0.02))
    _, so = o.solve(np.random.default_rng(1).normal(0, 1.0, (40, 3)))
    t = o.trace()
    lines, want = [], []
    n_rejected = n_unclamped = 0
    for k in range(1, len(t)):
        dcost, dx, rho = t[k, 2], t[k, 4], t[k, 5]
        if k == len(t) - 1 and so["termination"] in (0, 2):
            assert t[k, 6] == t[k - 1, 6]                    # the terminating step is never applied
            continue
        if dcost == 0.0 and dx == 0.0 and rho == 0.0:
            lines.append("I")
        elif rho > 1e-3:
            lines.append("A %s" % float(rho).hex())
            n_unclamped += rho < 0.937
        else:
            lines.append("R")
            n_rejected += 1
        want.append("%016x" % int(np.float64(t[k, 6]).view(np.uint64)))
    print("%d LM iterations, %d rejected, %d accepted below the 3 x clamp" % (so["num_iterations"], n_rejected, n_unclamped))
    assert n_rejected >= 5 and n_unclamped >= 5
    r = subprocess.run([_build(tmp_path), "replay", float(t[0, 6]).hex(), float(1e16).hex()], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == want
