"""The relative-translation filter on the device (gsfm_pos_filter_relative_translations, include/gsfm_pos.h) against the numpy restatement
(tests/translation_filter_reference.py).  Directions, statistics and projections within the bounds of their fp64 chains; from the
device's own projections on -- ordering, bad weights, decisions, pass and pick counts -- exactly."""
import ctypes as C

import numpy as np
import pytest

from globalsfmpy_amd import _abi, synth
from globalsfmpy_amd.solver import PositionProblem, SolverError, filter_relative_translations
from globalsfmpy_amd import loss_functions as lf

import translation_filter_reference as tfr

pytestmark = pytest.mark.gpu


def graph(n_cams, n_edges, seed=21, outliers=0.3, noise=0.01):
    return synth.make_position_graph(n_cams, n_edges, seed, outlier_frac=outliers, noise=noise)


def run(g, **kw):
    kw.setdefault("want_projections", True)
    return filter_relative_translations(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], **kw)


def check_exact(n_cams, ei, ej, keep, out, tolerance):
    """everything after the projections, bit for bit, on the device's own projections"""
    ref = tfr.filter_from_projections(n_cams, ei, ej, out["projections"], tolerance)
    worst = float(np.max(np.abs(ref["bad_weight"] - out["bad_weight"])))
    print("n_cams %d edges %d: passes %s picks %s, max |bad - ref| %.3e, kept %d / ref %d"
          % (n_cams, len(ei), out["num_passes"][:4], out["num_picks"][:4], worst, int(keep.sum()), int(ref["keep"].sum())))
    assert np.array_equal(ref["num_passes"], out["num_passes"].astype(np.int64))
    assert np.array_equal(ref["num_picks"], out["num_picks"].astype(np.int64))
    assert np.array_equal(ref["bad_weight"].view(np.uint64), out["bad_weight"].view(np.uint64))
    assert np.array_equal(ref["keep"], keep)
    assert out["n_kept"] == int(keep.sum())
    return ref


def test_directions_statistics_projections():
    g = graph(600, 8000)
    keep, out = run(g, num_iterations=48, tolerance=0.08)
    d = tfr.world_directions(g["edge_i"], g["rel_t"], g["rot_aa"])
    mean, var = tfr.mean_variance(d)
    E = d.shape[0]
    bound = 4.0 * E * 2.0 ** -53
    print("mean err", np.abs(out["mean"] - mean), "var err", np.abs(out["variance"] - var), "bounds", bound * 1.0, bound * 4.0)
    assert np.all(np.abs(out["mean"] - mean) <= bound * 1.0)       # unit rel_t: |d_c| <= 1
    assert np.all(np.abs(out["variance"] - var) <= bound * 4.0)    # (d_c - mean_c)^2 <= 4
    proj = d @ out["axes"].T
    tnorm = np.linalg.norm(g["rel_t"], axis=1, keepdims=True)
    err = np.abs(out["projections"] - proj) / (tnorm * 2.0 ** -52)
    print("projections: max error %.2f ulp of |t|" % err.max())
    assert err.max() <= 64.0


@pytest.mark.parametrize("n_cams,n_edges", [(10, 30), (200, 2000), (600, 8000), (2000, 20000)])
def test_ordering_and_bad_weights_exact(n_cams, n_edges):
    g = graph(n_cams, n_edges)
    keep, out = run(g, num_iterations=48, tolerance=0.08)
    check_exact(g["n_cams"], g["edge_i"], g["edge_j"], keep, out, 0.08)


def test_global_memory_path_exact():
    g = graph(9000, 60000)   # 28 B x 9000 cameras do not fit one workgroup's LDS
    keep, out = run(g, num_iterations=3, tolerance=0.08)
    check_exact(g["n_cams"], g["edge_i"], g["edge_j"], keep, out, 0.08)


def test_parallel_arcs_components_and_unused_cameras():
    g = graph(120, 900, seed=5)
    # parallel arcs: the first 60 pairs again, half of them reversed, with their own translations
    rng = np.random.default_rng(3)
    u = rng.standard_normal((60, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    ei = np.concatenate([g["edge_i"], g["edge_i"][:30], g["edge_j"][30:60]]).astype(np.uint32)
    ej = np.concatenate([g["edge_j"], g["edge_j"][:30], g["edge_i"][30:60]]).astype(np.uint32)
    rel = np.vstack([g["rel_t"], u])
    keep, out = filter_relative_translations(120, ei, ej, rel, g["rot_aa"], num_iterations=16, tolerance=0.08, want_projections=True)
    check_exact(120, ei, ej, keep, out, 0.08)
    # two components and cameras without an edge: a second graph on cameras 150.., cameras 120..149 and the last 10 unused
    h = graph(80, 500, seed=6)
    n = 240
    ei2 = np.concatenate([g["edge_i"], h["edge_i"] + 150]).astype(np.uint32)
    ej2 = np.concatenate([g["edge_j"], h["edge_j"] + 150]).astype(np.uint32)
    rel2 = np.vstack([g["rel_t"], h["rel_t"]])
    rot2 = np.zeros((n, 3)); rot2[:120] = g["rot_aa"]; rot2[150:230] = h["rot_aa"]
    keep, out = filter_relative_translations(n, ei2, ej2, rel2, rot2, num_iterations=16, tolerance=0.08, want_projections=True)
    check_exact(n, ei2, ej2, keep, out, 0.08)


@pytest.mark.parametrize("n_cams,n_edges", [(10, 30), (200, 2000)])
def test_noise_free_input_keeps_everything(n_cams, n_edges):
    g = synth.make_position_graph(n_cams, n_edges, 21)
    keep, out = run(g, num_iterations=48, tolerance=0.08)
    assert keep.all() and out["n_kept"] == n_edges
    assert int(out["num_picks"].sum()) == 0      # the arcs form a DAG: sources all the way
    check_exact(g["n_cams"], g["edge_i"], g["edge_j"], keep, out, 0.08)


@pytest.mark.parametrize("outliers", [0.3, 0.1])
def test_it_does_its_job(outliers):
    g = graph(600, 8000, seed=21, outliers=outliers, noise=0.01)
    keep, out = run(g, num_iterations=48, tolerance=0.08)
    ref = check_exact(g["n_cams"], g["edge_i"], g["edge_j"], keep, out, 0.08)
    is_out = g["is_outlier"]
    dropped_out, dropped_in = int((~ref["keep"] & is_out).sum()), int((~ref["keep"] & ~is_out).sum())
    print("outliers %.1f: dropped %d of %d outliers, %d of %d inliers; mean picks per projection %.0f"
          % (outliers, dropped_out, int(is_out.sum()), dropped_in, int((~is_out).sum()), out["num_picks"].mean()))
    assert dropped_out >= 0.5 * is_out.sum()
    assert dropped_in <= 0.1 * (~is_out).sum()


def test_determinism_and_axes():
    g = graph(600, 8000)
    k1, o1 = run(g, num_iterations=48, tolerance=0.08, seed=7)
    k2, o2 = run(g, num_iterations=48, tolerance=0.08, seed=7)
    for name in ("bad_weight", "mean", "variance", "axes", "projections", "num_passes", "num_picks"):
        assert o1[name].tobytes() == o2[name].tobytes(), name
    assert k1.tobytes() == k2.tobytes() and o1["n_kept"] == o2["n_kept"]
    assert np.allclose(np.linalg.norm(o1["axes"], axis=1), 1.0, rtol=0, atol=1e-15)   # three correctly rounded divisions, and this norm's own rounding
    _, o3 = run(g, num_iterations=48, tolerance=0.08, seed=8)
    assert not np.array_equal(o3["axes"], o1["axes"])
    k4, o4 = run(g, num_iterations=48, tolerance=0.08, axes=o1["axes"])
    for name in ("bad_weight", "axes", "projections", "num_passes", "num_picks"):
        assert o4[name].tobytes() == o1[name].tobytes(), name
    assert k4.tobytes() == k1.tobytes()
    # without proj_out the result is the same
    k5, o5 = run(g, num_iterations=48, tolerance=0.08, seed=7, want_projections=False)
    assert o5["projections"] is None and o5["bad_weight"].tobytes() == o1["bad_weight"].tobytes() and k5.tobytes() == k1.tobytes()


def test_errors_are_invalid_arg():
    g = graph(10, 30)
    with pytest.raises(SolverError, match="status 1"):
        bad = g["edge_j"].copy(); bad[3] = 10
        filter_relative_translations(10, g["edge_i"], bad, g["rel_t"], g["rot_aa"])
    with pytest.raises(SolverError, match="status 1"):
        bad = g["edge_j"].copy(); bad[5] = g["edge_i"][5]
        filter_relative_translations(10, g["edge_i"], bad, g["rel_t"], g["rot_aa"])
    with pytest.raises(SolverError, match="status 1"):
        filter_relative_translations(10, g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], num_iterations=0)
    lib = _abi.load_library()
    ei = np.ascontiguousarray(g["edge_i"], dtype=np.uint32); ej = np.ascontiguousarray(g["edge_j"], dtype=np.uint32)
    rel = np.ascontiguousarray(g["rel_t"]); rot = np.ascontiguousarray(g["rot_aa"])
    bad_w, keep = np.empty(30), np.empty(30, dtype=np.uint8)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    k8 = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    tail = (None, None, None, None, None, None, None)
    assert lib.gsfm_pos_filter_relative_translations(10, 30, None, u32(ej), dp(rel), dp(rot), 48, None, 1, 0.1, dp(bad_w), k8, *tail) == _abi.ERR_INVALID_ARG
    assert lib.gsfm_pos_filter_relative_translations(10, 30, u32(ei), u32(ej), None, dp(rot), 48, None, 1, 0.1, dp(bad_w), k8, *tail) == _abi.ERR_INVALID_ARG
    assert lib.gsfm_pos_filter_relative_translations(10, 30, u32(ei), u32(ej), dp(rel), None, 48, None, 1, 0.1, dp(bad_w), k8, *tail) == _abi.ERR_INVALID_ARG
    assert lib.gsfm_pos_filter_relative_translations(10, 30, u32(ei), u32(ej), dp(rel), dp(rot), 48, None, 1, 0.1, None, k8, *tail) == _abi.ERR_INVALID_ARG
    assert lib.gsfm_pos_filter_relative_translations(10, 30, u32(ei), u32(ej), dp(rel), dp(rot), 48, None, 1, 0.1, dp(bad_w), None, *tail) == _abi.ERR_INVALID_ARG
    # weights that could overflow the 63-bit sums
    with pytest.raises(SolverError, match="status 1"):
        filter_relative_translations(10, g["edge_i"], g["edge_j"], g["rel_t"] * 1e12, g["rot_aa"])
    assert lib.gsfm_pos_filter_relative_translations(10, 30, u32(ei), u32(ej), dp(rel), dp(rot), 48, None, 1, 0.1, dp(bad_w), k8, *tail) == _abi.OK


def test_downstream_position_solve_before_and_after():
    """Recorded, not gated beyond sanity: the position solve on the largest component before and after the filter."""
    g = graph(600, 8000, seed=21, outliers=0.3, noise=0.01)
    keep, out = run(g, num_iterations=48, tolerance=0.08, want_projections=False)

    def solve(mask):
        ei, ej, rel = g["edge_i"][mask], g["edge_j"][mask], g["rel_t"][mask]
        # largest component of the kept edges
        parent = np.arange(g["n_cams"])
        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]; x = parent[x]
            return x
        for a, b in zip(ei, ej):
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[ra] = rb
        roots = np.array([find(v) for v in range(g["n_cams"])])
        used = np.zeros(g["n_cams"], dtype=bool); used[ei] = True; used[ej] = True
        vals, counts = np.unique(roots[used], return_counts=True)
        big = vals[np.argmax(counts)]
        cams = np.flatnonzero(used & (roots == big))
        index = -np.ones(g["n_cams"], dtype=np.int64); index[cams] = np.arange(cams.size)
        m = (roots[ei] == big)
        p = PositionProblem(cams.size, index[ei[m]].astype(np.uint32), index[ej[m]].astype(np.uint32), rel[m], g["rot_aa"][cams])
        p.set_loss(lf.HuberLoss(0.1))
        x, s = p.solve(None, fixed_cam=0)
        err = np.linalg.norm(synth.gauge_normalize(x, 0) - synth.gauge_normalize(g["gt_pos"][cams], 0), axis=1)
        return cams.size, int(m.sum()), s, err

    for name, mask in (("unfiltered", np.ones(keep.size, dtype=bool)), ("filtered", keep)):
        n, e, s, err = solve(mask)
        print("%s: %d cameras %d edges, final cost %.6e, LM %d, PCG %d, dense %d, median err %.3e, mean err %.3e, max err %.3e"
              % (name, n, e, s["final_cost"], s["num_iterations"], s["num_cg_iterations"], s["num_dense_solves"], np.median(err), err.mean(), err.max()))
        assert np.isfinite(s["final_cost"]) and not s["nonfinite"]
