"""-m gpu: the column-sorted mat-vec (K3c, csrc/colsort_kernels.hpp: k_mv_col + k_mv_col_finish) on the shapes where its sub-chunk loop,
its row phase and its record formats can go wrong, against the high-precision reference (tests/hp_reference.py) with the rounding bounds
of tests/test_gpu_hp_linearization.py:

    |y_dev - y*| <= (16 + deg(k)) u sum_e |J~_e|^T |J~_e| |v|     per component, and the median row's bound allows <= 1e-11 relative.

Every case runs with the 2-byte delta-coded record (GSFM_K3C_K16=1) and with the 4-byte one (GSFM_K3C_K16=0); the two products must be
bit-equal (the same numbers added in the same order).

The reference costs ~7 ms per edge (mpmath), so the graphs are built from a POOL: eight camera rotations and, per ordered pair of them,
three error rotations -- 192 distinct edges, evaluated once per module by hp_reference.edge_set; a case's cameras draw their rotation
from the pool and its edges index the table.  Nothing of the device's arithmetic knows about the pool: every entry is linearised,
stored and multiplied on its own.

Shapes (rows come in blocks of 512, a block's entries in sub-chunks of 512 positions, dealt to the block's workgroups):
  wgs2 / wgs4 / wgs10   600 cameras, 1 500 edges, GSFM_COL_WGS = 2, 4, 10: tasks of 5 and 1, of 2-3 and 0-1, of 1 and 0 sub-chunks
  one_row_block         513 cameras: the second block is a single row, most of its tasks hold no sub-chunk and write zero partials
  ragged                1 100 cameras, 20 000 edges: a ragged last block, padding at the end of every block's last sub-chunk
  hub                   8 000 cameras, 6 000 edges and a hub camera with 3 000 more: camera steps >= 15 and row counts >= 7 (both escapes
                        of the 2-byte record), rows with hundreds of slots in one sub-chunk (the rolled slot loop)
"""

import numpy as np
import pytest

from globalsfmpy_amd import _abi
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem

import hp_reference as H
from test_gpu_hp_linearization import ALLOW_MEDIAN, CA, U, _aa, _rel_for
from test_gpu_loss_golden import _assert_rows
from test_oracle_golden import _cases

pytestmark = pytest.mark.gpu

ET = _abi.ANGLE_AXIS
P, V = 8, 3          # pool: camera rotations, error rotations per ordered pair
FORCED = {"GSFM_K3_COLSORT": "1", "GSFM_PCG_COARSE": "0", "GSFM_REORDER": "0"}


@pytest.fixture(scope="module")
def pool():
    """The pool's rotations, the 192 distinct edges and their reference linearisation (no loss), computed once and never changed."""
    rng = np.random.default_rng(17)
    rot = np.array([_aa(rng.uniform(0.2, 2.8), rng.standard_normal(3)) for _ in range(P)])
    thetas = (0.02, 0.3, 1.0)
    a, b = np.divmod(np.arange(P * P * V) // V, P)
    rel = np.array([_rel_for(rot[i], rot[j], _aa(thetas[k % V], rng.standard_normal(3))) for k, (i, j) in enumerate(zip(a, b))])
    lin = H.corrected(H.edge_set(ET, a, b, rel, rot))
    for v in lin.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return {"rot": rot, "rel": rel, "lin": lin}


def _graph(pool, n, edges, seed):
    """Cameras with pool rotations, the given (i, j) pairs with pool measurements; the reference rows of its edges."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, P, n)
    ei, ej = np.asarray(edges[0]), np.asarray(edges[1])
    idx = (kind[ei] * P + kind[ej]) * V + rng.integers(0, V, len(ei))
    lin = {k: (v[:, idx] if k == "rho" else v[idx]) for k, v in pool["lin"].items()}   # (rho is 3 x E, everything else E x ...)
    return {"n": n, "ei": ei, "ej": ej, "rel": pool["rel"][idx], "rot": pool["rot"][kind], "lin": lin}


def _random_edges(n, m, seed):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, m)
    ej = (ei + 1 + rng.integers(0, n - 1, m)) % n
    return ei, ej


def _hub_edges():
    n = 8000
    ei, ej = _random_edges(n, 6000, 5)
    others = np.random.default_rng(6).choice(n, 3000, replace=False)
    hub = np.full(3000, 4000)   # (a camera in the middle of a block)
    others = np.where(others == 4000, 4001, others)
    return n, (np.concatenate([ei, hub[:1500], others[1500:]]), np.concatenate([ej, others[:1500], hub[1500:]]))


CASES = {
    "wgs2": (lambda: (600, _random_edges(600, 1500, 1)), {"GSFM_COL_WGS": "2"}),
    "wgs4": (lambda: (600, _random_edges(600, 1500, 1)), {"GSFM_COL_WGS": "4"}),
    "wgs10": (lambda: (600, _random_edges(600, 1500, 1)), {"GSFM_COL_WGS": "10"}),
    "one_row_block": (lambda: (513, _random_edges(513, 1500, 2)), {}),
    "ragged": (lambda: (1100, _random_edges(1100, 20000, 3)), {}),
    "hub": (_hub_edges, {}),
}


def _problem(monkeypatch, g, env, k16):
    for k, v in dict(FORCED, GSFM_K3C_K16=k16, **env).items():
        monkeypatch.setenv(k, v)
    dev = RotationProblem(g["n"], g["ei"], g["ej"], g["rel"], ET)
    assert dev.matvec_bytes()[1] == 2, "the column-sorted form was not built"
    return dev


@pytest.mark.parametrize("case", sorted(CASES))
def test_products_against_hp_reference_and_between_record_formats(pool, monkeypatch, case):
    make, env = CASES[case]
    n, edges = make()
    g = _graph(pool, n, edges, 11)
    deg = np.bincount(g["ei"], minlength=n) + np.bincount(g["ej"], minlength=n)
    if case == "hub":
        assert deg.max() >= 3000
    ck = H.c_row(deg, CA)
    rng = np.random.default_rng(3)
    vs = {"mv_unit": np.eye(3)[np.arange(n) % 3], "mv_rand": rng.standard_normal((n, 3))}
    got = {}
    for k16 in ("1", "0"):
        dev = _problem(monkeypatch, g, env, k16)
        dev.linearize(g["rot"])
        got[k16] = {name: dev.normal_matvec(v) for name, v in vs.items()}
        dev.close()
    for name, v in vs.items():
        y, ym, yt = H.matvec(g["lin"], n, g["ei"], g["ej"], v)
        bound = ck[:, None] * U * ym
        worst = {k16: H.ratio(got[k16][name], y, bound) for k16 in got}
        allow = H.allowed_relative(bound, yt)
        print("%s %s worst |err| / bound: 2-byte record %.3e, 4-byte %.3e; median allowed relative %.1e" % (case, name, worst["1"], worst["0"], allow))
        assert worst["1"] <= 1.0 and worst["0"] <= 1.0, (case, name, worst)
        assert allow <= ALLOW_MEDIAN, ("vacuous bound", case, name, allow)
        assert np.array_equal(got["1"][name], got["0"][name]), (case, name, "the record formats disagree")


@pytest.mark.parametrize("case", ["wgs4", "hub"])
@pytest.mark.parametrize("single", [0, 1])
def test_four_lm_iterations_agree_between_record_formats(pool, monkeypatch, case, single):
    make, env = CASES[case]
    n, edges = make()
    g = _graph(pool, n, edges, 11)
    out = {}
    for k16 in ("1", "0"):
        dev = _problem(monkeypatch, g, env, k16)
        out[k16] = dev.solve(g["rot"], max_num_iterations=4, pcg_single_reduction=single, dense_cholesky_max_cams=0)
        dev.close()
    (r1, s1), (r0, s0) = out["1"], out["0"]
    assert s1["num_cg_iterations"] > 0
    assert np.array_equal(r1, r0)
    assert s1["num_cg_iterations"] == s0["num_cg_iterations"] and s1["num_iterations"] == s0["num_iterations"]
    assert s1["final_cost"] == s0["final_cost"]


def test_magsac_cost_only_value_against_the_recorded_rows(golden_dir):
    """loss_value<LM_MAGSAC> (the trial-cost sweeps and the fused trial linearisation) is the nu = 3, non-inverted value function chosen at
    compile time: the recorded rows of MAGSACWeightBasedLoss(0.02), at the bar of tests/test_gpu_loss_golden.py."""
    case = next(c for c in _cases(golden_dir) if c["class"] == "MAGSACWeightBasedLoss" and tuple(c["args"]) == (0.02, False) and not c["program"])
    rows = np.asarray(case["rows"], dtype=np.float64)
    assert len(rows) > 20
    dev = RotationProblem(8, np.arange(7), np.arange(1, 8), np.zeros((7, 3)), ET)
    dev.set_loss(LF.MAGSACWeightBasedLoss(0.02))
    _, val = dev.loss_eval(rows[:, 0])
    _assert_rows(val[:, None], rows[:, :2], 1e-12, "MAGSAC(0.02) value")
    dev.close()
