"""The numpy restatement of the relative-translation filter (tests/translation_filter_reference.py) against a second, naive implementation
that follows Theia's filter_view_pairs_from_relative_translation.cc step by step with Python dicts -- one node per pass, sources taken in
ascending index -- and on Theia's own test cases.  No device."""
import numpy as np
import pytest

from globalsfmpy_amd import synth

import translation_filter_reference as tfr

TWO32 = 1 << 32


def naive_ordering(edge_i, edge_j, p):
    """OrderTranslationsFromProjections with dicts: degrees_for_view of MFAS nodes, FindNextViewInOrder (a source if there is one -- the
    smallest index here, where the reference takes the first its hash map meets --, else the largest (out + 1) / (in + 1) in the integer
    scale of the definition, the smallest index among equals), one view per step.  Returns view -> position in the order."""
    q = [int(x) for x in tfr.arc_weights(np.asarray(p))]
    nodes = {}
    for e, (i, j) in enumerate(zip(edge_i, edge_j)):
        a, b = (int(i), int(j)) if p[e] > 0 else (int(j), int(i))   # the arc a -> b
        for v in (a, b):
            nodes.setdefault(v, {"in": {}, "out": {}, "win": 0, "wout": 0})
        nodes[b]["win"] += q[e]
        nodes[a]["wout"] += q[e]
        nodes[b]["in"].setdefault(a, []).append(q[e])    # (a repeated pair: parallel arcs)
        nodes[a]["out"].setdefault(b, []).append(q[e])
    order = {}
    for step in range(len(nodes)):
        best, best_score = None, 0.0
        for v in sorted(nodes):
            if len(nodes[v]["in"]) == 0:
                best = v
                break
            score = float(nodes[v]["wout"] + TWO32) / float(nodes[v]["win"] + TWO32)
            if score > best_score:
                best, best_score = v, score
        order[best] = step
        info = nodes.pop(best)
        for m, ws in info["in"].items():
            nodes[m]["wout"] -= sum(ws)
            del nodes[m]["out"][best]
        for m, ws in info["out"].items():
            nodes[m]["win"] -= sum(ws)
            del nodes[m]["in"][best]
    return order


def naive_inconsistent(edge_i, edge_j, p):
    order = naive_ordering(edge_i, edge_j, p)
    out = np.zeros(len(edge_i), dtype=bool)
    for e, (i, j) in enumerate(zip(edge_i, edge_j)):
        diff = order[int(j)] - order[int(i)]
        out[e] = (diff < 0 and p[e] > 0) or (diff > 0 and p[e] < 0)
    return out


@pytest.mark.parametrize("n_cams,n_edges,seed,outliers,noise", [
    (4, 6, 1, 0.3, 0.05), (10, 30, 2, 0.3, 0.01), (25, 120, 3, 0.3, 0.01), (40, 300, 4, 0.5, 0.05), (60, 500, 5, 0.3, 0.01),
    (60, 900, 6, 0.8, 0.1), (30, 100, 7, 0.0, 0.0),
])
def test_all_sources_per_pass_changes_nothing(n_cams, n_edges, seed, outliers, noise):
    """Step 6's claim: removing all sources of a pass at once leaves every edge on the same side as removing them one at a time."""
    g = synth.make_position_graph(n_cams, n_edges, seed, outlier_frac=outliers, noise=noise)
    ref = tfr.filter_relative_translations(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], num_iterations=12, tolerance=0.08, seed=seed)
    for k in range(12):
        p = ref["projections"][:, k]
        assert np.array_equal(ref["inconsistent"][:, k], naive_inconsistent(g["edge_i"], g["edge_j"], p)), "projection %d" % k


def test_parallel_arcs_and_components():
    rng = np.random.default_rng(11)
    ei = np.array([0, 0, 1, 2, 0, 5, 6, 5, 5, 1], dtype=np.uint32)
    ej = np.array([1, 1, 2, 0, 2, 6, 7, 7, 6, 0], dtype=np.uint32)   # (0, 1) twice and (1, 0): parallel arcs; {5, 6, 7} apart; 3, 4, 8 unused
    for trial in range(20):
        p = rng.standard_normal(ei.size)
        passes, n_pass, n_pick = tfr.order_passes(9, tfr.build_rows(9, ei, ej), p)
        assert np.all(passes[[3, 4, 8]] == -1) and np.all(passes[[0, 1, 2, 5, 6, 7]] >= 0)
        assert np.array_equal(tfr.inconsistent_edges(ei, ej, p, passes), naive_inconsistent(ei, ej, p))


def line_graph():
    """Theia's LineTest: four cameras on the x axis, zero orientations, the chain's three edges and the bad edge (0, 3)."""
    ei = np.array([0, 1, 2, 0], dtype=np.uint32)
    ej = np.array([1, 2, 3, 3], dtype=np.uint32)
    rel_t = np.array([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], list(-np.ones(3) / np.sqrt(3.0))])
    return 4, ei, ej, rel_t, np.zeros((4, 3))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 7])
def test_line_bad_edge_dropped(seed):
    n, ei, ej, rel_t, rot = line_graph()
    ref = tfr.filter_relative_translations(n, ei, ej, rel_t, rot, num_iterations=48, tolerance=0.1, seed=seed)
    assert not ref["keep"][3]


def test_line_only_bad_edge_dropped():
    n, ei, ej, rel_t, rot = line_graph()
    only = [s for s in range(40) if list(tfr.filter_relative_translations(n, ei, ej, rel_t, rot, 48, 0.1, seed=s)["keep"]) == [True, True, True, False]]
    assert only, "no seed of 0..39 drops (0, 3) alone"
    ref = tfr.filter_relative_translations(n, ei, ej, rel_t, rot, 48, 0.1, seed=only[0])
    assert list(ref["keep"]) == [True, True, True, False]


def theia_case(num_views, num_valid, num_invalid, seed):
    """TestFilterViewPairsFromRelativeTranslation's input: random poses, a chain plus random valid pairs, invalid pairs with random unit
    translations."""
    rng = np.random.default_rng(seed)
    rot = rng.uniform(-1, 1, (num_views, 3)); rot[0] = 0
    pos = rng.uniform(-1, 1, (num_views, 3)); pos[0] = 0
    pairs = [(i - 1, i) for i in range(1, num_views)]
    have = set(pairs)
    while len(pairs) < num_valid:
        a, b = rng.choice(num_views, 2, replace=False)
        if a > b or (a, b) in have:
            continue
        pairs.append((int(a), int(b))); have.add((int(a), int(b)))
    ei = np.array([a for a, _ in pairs], dtype=np.int64); ej = np.array([b for _, b in pairs], dtype=np.int64)
    d = pos[ej] - pos[ei]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rel = np.einsum("eij,ej->ei", synth.aa_to_matrix(rot[ei]), d)
    bad = []
    while len(bad) < num_invalid:
        a, b = rng.integers(0, num_views, 2)
        if a >= b or (int(a), int(b)) in have:
            continue
        bad.append((int(a), int(b))); have.add((int(a), int(b)))
    u = rng.standard_normal((num_invalid, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ei = np.concatenate([ei, np.array([a for a, _ in bad], dtype=np.int64)]).astype(np.uint32)
    ej = np.concatenate([ej, np.array([b for _, b in bad], dtype=np.int64)]).astype(np.uint32)
    return num_views, ei, ej, np.vstack([rel, u.reshape(-1, 3)]), rot


@pytest.mark.parametrize("views,valid,invalid", [(10, 30, 0), (10, 30, 5), (30, 100, 30)])
def test_theia_random_cases_keep_the_good_pairs(views, valid, invalid):
    n, ei, ej, rel_t, rot = theia_case(views, valid, invalid, seed=169)
    ref = tfr.filter_relative_translations(n, ei, ej, rel_t, rot, num_iterations=48, tolerance=0.08, seed=169)
    assert int(ref["keep"].sum()) >= valid


def test_noise_free_input_is_a_dag():
    for n_cams, n_edges in [(10, 30), (200, 2000)]:
        g = synth.make_position_graph(n_cams, n_edges, 3)
        ref = tfr.filter_relative_translations(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], 48, 0.08, seed=1)
        assert ref["keep"].all() and int(ref["num_picks"].sum()) == 0
