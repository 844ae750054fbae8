"""The exact step's failure and rest paths end to end: a factorisation that breaks down hands the whole LM step back to PCG -- on a connected
graph under both LM controls, and on a disconnected graph whose components are all factorised side by side -- without a NaN or an inf from
the failed factor reaching the per-component step measurement; and the rule that puts a converged component to rest does not put a scene
to rest whose step is small only because the damping makes it so."""
import re

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem
from test_gpu_round5 import _batch_of_scenes

pytestmark = pytest.mark.gpu

# a trust region of 1e20: the damping vanishes and every normal matrix keeps its gauge null space, so the factorisation meets a non-positive
# pivot (test_gpu_parity.py, test_a_factorisation_that_breaks_down_is_solved_again_by_pcg); pcg_forcing=0: exact steps on both sides
BREAKDOWN = dict(initial_trust_region_radius=1e20, max_trust_region_radius=1e20, pcg_forcing=0)


@pytest.mark.parametrize("control", [1, 0])
def test_connected_breakdown_falls_back_under_both_controls(control):
    g = synth.make_graph(60, 400, 3, outlier_frac=0.1)
    p = RotationProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], _abi.ANGLE_AXIS); p.set_loss(LF.HuberLoss(0.1))
    rd, sd = p.solve(g["init_aa"], lm_device_control=control, **BREAKDOWN)
    rp, sp = p.solve(g["init_aa"], lm_device_control=control, dense_cholesky_max_cams=0, **BREAKDOWN)
    print("control %d: %d LM it, %d exact steps, %d sweeps (PCG only: %d it, %d sweeps)" % (
        control, sd["num_iterations"], sd["num_dense_solves"], sd["num_residual_sweeps"], sp["num_iterations"], sp["num_residual_sweeps"]))
    assert sd["termination_name"] == sp["termination_name"] == "FUNCTION_TOLERANCE" and not sd["nonfinite"]
    assert sd["num_dense_solves"] < sd["num_iterations"] and sd["num_cg_iterations"] > 0
    assert sd["num_residual_sweeps"] == sp["num_residual_sweeps"]
    assert abs(sd["final_cost"] - sp["final_cost"]) <= 1e-6 * sp["final_cost"]
    assert synth.angular_distance(synth.align_rotations(rd, rp), rp).mean() <= 1e-4


def _component_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("[gsfm] components:")]


def test_disconnected_breakdown_falls_back_and_measures_no_nan(capfd):
    """Every component at most 512 cameras (no PCG beside the factorisations): a component's factor breaks down, the step is solved again by
    PCG, and the failed item's garbage (NaN / inf in its x) never reaches the step measurement of the rest rule (k_comp_scatter skips it:
    the verbose line marks it `bad:` with nothing measured).  Each component ends where the PCG-only solve ends."""
    sizes = (200, 260, 150, 90)
    N, ei, ej, rel, cov, init, comp = _batch_of_scenes(sizes, 700)
    dev = RotationProblem(N, ei, ej, rel, _abi.ANGLE_AXIS_COVTRACE, cov6=cov); dev.set_loss(LF.HuberLoss(0.1))
    capfd.readouterr()
    rd, sd = dev.solve(init, verbose=1, **BREAKDOWN)
    err = capfd.readouterr().err
    rp, sp = dev.solve(init, dense_cholesky_max_cams=0, **BREAKDOWN)
    lines = _component_lines(err)
    print("\n".join(lines[:4]))
    print("%d LM it, %d component steps (PCG only: %d it)" % (sd["num_iterations"], sd["num_dense_solves"], sp["num_iterations"]))
    assert sd["num_dense_solves"] < sd["num_iterations"] and not sd["nonfinite"]          # at least one step fell back
    assert sd["termination_name"] == sp["termination_name"] and sd["num_iterations"] == sp["num_iterations"]
    assert abs(sd["final_cost"] - sp["final_cost"]) <= 1e-9 * sp["final_cost"]
    for c in range(len(sizes)):
        m = comp == c
        assert synth.angular_distance(synth.align_rotations(rd[m], rp[m]), rp[m]).mean() <= 1e-6, c
    # the invariant: after a failed factorisation no live component shows a NaN or an inf (idle ones show +inf: nothing measured)
    assert lines and any("bad:" in ln for ln in lines), err[-2000:]
    for ln in lines:
        for tok in ln.split(":", 1)[1].split("(")[0].split():
            if not tok.startswith("idle:"):
                assert not re.search(r"nan|inf", tok, re.I), ln


def _tokens(line):
    return line.split(":", 1)[1].split("(")[0].split()


def test_a_damped_small_step_does_not_put_a_scene_to_rest(oracle, capfd):
    """Two scenes under Huber, 600 cameras in all (more than dense_cholesky_max_cams: the component path, each scene factorised on its own):
    scene A from its synthetic start, scene B from the oracle's optimum for B moved by ~1e-5 rad per camera, and a small initial trust radius
    (1e-6; function_tolerance 1e-10 keeps the reference running at that radius).  B's first exact step is below the 1e-10 rad threshold
    because the damping makes it so -- a damped step scales with the radius -- not because B has converged.  The rule of round 6 (a step
    below the threshold while the radius is at or above the caller's initial one) put B to rest after that step, ~1e-5 rad off; the rest rule
    (comp_rest.hpp) asks for a weak damping or a contraction at a non-shrinking radius, and B converges with A, within the bar of the oracle,
    as with component_rest=0."""
    sizes = (450, 150)
    N, ei, ej, rel, cov, init, comp = _batch_of_scenes(sizes, 900)
    assert N > 512
    loss = LF.HuberLoss(0.1)
    mB = comp == 1
    off = int(np.flatnonzero(mB)[0])
    eB = comp[ei] == 1
    oB = oracle.OracleProblem(int(mB.sum()), ei[eB] - off, ej[eB] - off, rel[eB], _abi.ANGLE_AXIS_COVTRACE, cov6=cov[eB]); oB.set_loss(loss)
    rB, _ = oB.solve(init[mB], function_tolerance=1e-16, parameter_tolerance=1e-16, gradient_tolerance=1e-30)
    d = np.random.default_rng(1).standard_normal(rB.shape)
    start = init.copy()
    start[mB] = rB + 1e-5 * d / np.linalg.norm(d, axis=1).mean()
    kw = dict(initial_trust_region_radius=1e-6, function_tolerance=1e-10)
    ora = oracle.OracleProblem(N, ei, ej, rel, _abi.ANGLE_AXIS_COVTRACE, cov6=cov); ora.set_loss(loss)
    ro, so = ora.solve(start, **kw)
    dev = RotationProblem(N, ei, ej, rel, _abi.ANGLE_AXIS_COVTRACE, cov6=cov); dev.set_loss(loss)
    out = {}
    for rest in (1, 0):
        capfd.readouterr()
        r, s = dev.solve(start, component_rest=rest, verbose=1, **kw)
        lines = _component_lines(capfd.readouterr().err)
        errs = [synth.angular_distance(synth.align_rotations(r[comp == c], ro[comp == c]), ro[comp == c]).mean() for c in range(len(sizes))]
        out[rest] = (s, errs, lines)
    for rest, (s, errs, lines) in out.items():   # (after the loop: capfd takes what is printed between two reads)
        print("component_rest %d: %d LM it (oracle %d), %s; mean |dR| per scene %s; B's steps %s" % (
            rest, s["num_iterations"], so["num_iterations"], s["termination_name"], " ".join("%.2e" % e for e in errs),
            " ".join(_tokens(ln)[1] for ln in lines[:8])))
    s1, _, lines = out[1]
    # the scenario: B is factorised, and its first exact step is a damped one below the threshold (what the rule of round 6 rested)
    assert len(lines) >= 2 and all(len(_tokens(ln)) == 2 for ln in lines)
    first_B = _tokens(lines[0])[1]
    assert not first_B.startswith(("idle:", "rest:")) and float(first_B) <= 1e-10, lines[0]
    assert not _tokens(lines[1])[1].startswith("rest:"), lines[1]
    assert so["num_iterations"] > 5
    for rest, (s, errs, _) in out.items():
        assert s["num_iterations"] == so["num_iterations"] and s["termination_name"] == so["termination_name"], rest
        for c, e in enumerate(errs):
            assert e <= 1e-6, (rest, c, e)
