"""The rotation problem orders every fill and copy of its memory on its own stream (csrc/host_common.hpp, DevBuf).  What a solve finds in
buffers that are allocated and cleared at first use -- the dense tiles, the callback-loss planes, the weight planes, the sigma-consensus
table, the component batch, the column-sorted layout -- must not depend on what ran on the problem before, or on when the host arrays they
were filled from died: every pairing below is compared bit for bit."""
import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import RotationProblem

pytestmark = pytest.mark.gpu


class PyMagsac(object):
    """a loss the device only reaches through the host callback (no native_program)"""

    def __init__(self, sigma):
        self.inner = LF.MAGSACWeightBasedLoss(sigma)

    def Evaluate(self, s, out):
        self.inner.Evaluate(s, out)


@pytest.fixture(scope="module")
def graph():
    return synth.make_graph(60, 400, seed=7, outlier_frac=0.1)


def _problem(g, et, loss=None):
    p = RotationProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_aa"], et, cov6=g["cov6"])
    p.set_loss(loss)
    return p


def _same_solve(a, b, keys=()):
    (ra, sa), (rb, sb) = a, b
    assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64))
    for k in ("num_iterations", "termination", "final_cost") + tuple(keys):
        assert sa[k] == sb[k], (k, sa, sb)


def test_one_problem_object_across_its_lazily_allocating_paths(graph):
    """PCG, then the dense step (its tiles allocated and cleared at first use), then a host-callback loss (its buffers allocated at first
    use; PCG steps again, so that the exact step is taken in the dense case alone) on ONE problem object: each solve equals, bit for bit,
    the same solve on a fresh problem."""
    g, et = graph, _abi.ANGLE_AXIS_COVARIANCE
    p = _problem(g, et, LF.MAGSACWeightBasedLoss(0.02))
    for case, loss, kw in (("pcg", None, {"dense_cholesky_max_cams": 0}), ("dense", None, {}), ("callback", PyMagsac(0.02), {"dense_cholesky_max_cams": 0})):
        if loss is not None:
            p.set_loss(loss)
        fresh = _problem(g, et, loss if loss is not None else LF.MAGSACWeightBasedLoss(0.02))
        one, other = p.solve(g["init_aa"], **kw), fresh.solve(g["init_aa"], **kw)
        _same_solve(one, other)
        assert (one[1]["num_dense_solves"] > 0) == (case == "dense"), (case, one[1])
        fresh.close()
    p.close()


def test_edge_weights_then_sigma_consensus_twice(graph):
    """set_edge_weights promotes a plain ANGLE_AXIS problem to scalar weights; two sigma-consensus solves on the same object then equal the
    same two calls on a fresh problem, weight change and outer iterations included."""
    g = graph
    w = np.random.default_rng(3).uniform(0.2, 3.0, size=g["edge_i"].shape[0])
    out = []
    for _ in range(2):
        p = _problem(g, _abi.ANGLE_AXIS)
        p.set_edge_weights(w)
        out.append([p.solve_sigma_consensus(g["init_aa"], 3, 0.02) for _call in range(2)])
        p.close()
    for call in range(2):
        _same_solve(out[0][call], out[1][call], keys=("last_weight_change", "outer_iterations"))


def test_components_built_at_first_use():
    """Two disjoint graphs and a camera without edges: the component batch is built inside the first solve."""
    a, b = synth.make_graph(30, 150, seed=11), synth.make_graph(30, 150, seed=12)
    g = {"n_cams": 61, "edge_i": np.concatenate([a["edge_i"], b["edge_i"] + 30]).astype(np.uint32),
         "edge_j": np.concatenate([a["edge_j"], b["edge_j"] + 30]).astype(np.uint32), "rel_aa": np.concatenate([a["rel_aa"], b["rel_aa"]]),
         "cov6": np.concatenate([a["cov6"], b["cov6"]])}
    init = np.concatenate([a["init_aa"], b["init_aa"], [[0.1, -0.2, 0.3]]])
    out = []
    for _ in range(2):
        p = _problem(g, _abi.ANGLE_AXIS_COVARIANCE, LF.MAGSACWeightBasedLoss(0.02))
        out.append(p.solve(init))
        p.close()
    _same_solve(out[0], out[1])
    assert out[0][1]["num_dense_solves"] > 0, out[0][1]
    assert np.array_equal(out[0][0][60], init[60])


def test_column_sorted_layout_at_the_smallest_size_that_builds_it(monkeypatch):
    """GSFM_K3_COLSORT=1 forces the layout: its host arrays are uploaded asynchronously and must outlive the copies."""
    g = synth.make_graph(300, 3000, seed=5)
    out = {}
    for key, mode in (("a", "1"), ("b", "1"), ("rows", None)):
        if mode is None:
            monkeypatch.delenv("GSFM_K3_COLSORT", raising=False)
        else:
            monkeypatch.setenv("GSFM_K3_COLSORT", mode)
        p = _problem(g, _abi.ANGLE_AXIS_COVTRACE)
        assert p.matvec_bytes()[1] == (2 if mode else 1)
        out[key] = p.solve(g["init_aa"], dense_cholesky_max_cams=0)
        p.close()
    _same_solve(out["a"], out["b"])
    # (the bar of test_gpu_round3.py::test_column_sorted_matvec_equals_the_row_major_form)
    c0, c1 = out["rows"][1]["final_cost"], out["a"][1]["final_cost"]
    assert abs(c0 - c1) <= 1e-11 * c0, (c0, c1)
