"""The host layer of the relative-translation filter: theia::FilterViewPairsFromRelativeTranslation and
GlobalReconstructionEstimator.FilterRelativeTranslation() on a synthetic view graph remove exactly the edges the flat call marks, then
the views that lost their component; with the YAML switch off the graph is unchanged."""
import os
import sys

import numpy as np
import pytest

from globalsfmpy_amd import synth
from globalsfmpy_amd.solver import filter_relative_translations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # where the compiled module lives, as the reference's scripts append ../build

pytestmark = pytest.mark.gpu


def _sfm():
    from globalsfmpy_amd import GlobalSfMpy as sfm
    return sfm


def build(sfm, g, ids, extra_view=None):
    vg = sfm.ViewGraph()
    for i, j, t in zip(g["edge_i"], g["edge_j"], g["rel_t"]):
        info = sfm.TwoViewInfo()
        info.position_2 = t
        vg.AddEdge(int(ids[i]), int(ids[j]), info)
    o = sfm.MapViewIdVector3d()
    for k in range(g["n_cams"]):
        o[int(ids[k])] = g["rot_aa"][k]
    if extra_view is not None:   # an edge whose first view has no orientation: skipped and kept
        lone = sfm.TwoViewInfo()
        lone.position_2 = np.array([0.0, 1.0, 0.0])
        vg.AddEdge(int(extra_view), int(extra_view) + 1, lone)
    return vg, o


def flat_marks(vg, o, num_iterations, tolerance, seed):
    """the shim's flattening: views ranked by id, the pairs whose first view has an orientation in sorted order"""
    ids = sorted(int(v) for v in vg.ViewIds())
    index = {v: k for k, v in enumerate(ids)}
    pairs = vg.GetAllEdges()
    keys = sorted(k for k in pairs.keys() if k[0] in o)
    ei = np.array([index[k[0]] for k in keys], dtype=np.uint32)
    ej = np.array([index[k[1]] for k in keys], dtype=np.uint32)
    rel = np.array([pairs[k].position_2 for k in keys]).reshape(-1, 3)
    rot = np.array([o[v] if v in o else np.zeros(3) for v in ids])
    keep, _ = filter_relative_translations(len(ids), ei, ej, rel, rot, num_iterations=num_iterations, tolerance=tolerance, seed=seed)
    return keys, keep


def components(edges):
    parent = {}
    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for a, b in edges:
        parent[find(a)] = find(b)
    groups = {}
    for v in list(parent):
        groups.setdefault(find(v), set()).add(v)
    return sorted(groups.values(), key=lambda s: (-len(s), min(s)))


def test_cpp_function_removes_the_marked_edges():
    sfm = _sfm()
    g = synth.make_position_graph(150, 1200, seed=4, outlier_frac=0.3, noise=0.01)
    ids = np.arange(150) * 3 + 1
    vg, o = build(sfm, g, ids, extra_view=5000)
    keys, keep = flat_marks(vg, o, 48, 0.08, 5)
    assert 0 < int((~keep).sum()) < keep.size
    before = set(vg.GetAllEdges().keys())
    opts = sfm.FilterViewPairsFromRelativeTranslationOptions()
    assert opts.num_iterations == 48 and opts.translation_projection_tolerance == 0.08
    opts.seed = 5
    opts.num_threads = 8   # accepted and ignored
    sfm.FilterViewPairsFromRelativeTranslation(opts, o, vg)
    after = set(vg.GetAllEdges().keys())
    assert before - after == {k for k, kp in zip(keys, keep) if not kp}
    assert (5000, 5001) in after


def estimator_graph(sfm):
    g = synth.make_position_graph(150, 700, seed=8, outlier_frac=0.4, noise=0.01)
    ids = np.arange(150) * 2 + 10
    vg, o = build(sfm, g, ids)
    return g, ids, vg, o


def test_estimator_method_filters_and_drops_lost_views(tmp_path):
    sfm = _sfm()
    g, ids, vg, o = estimator_graph(sfm)
    options = sfm.ReconstructionEstimatorOptions()
    assert options.filter_relative_translations_with_1dsfm is True
    assert options.translation_filtering_num_iterations == 48 and options.translation_filtering_projection_tolerance == 0.1
    options.translation_filtering_projection_tolerance = 0.02   # tight: enough edges go for some views to lose the component
    est = sfm.GlobalReconstructionEstimator(options)
    scene = sfm.Reconstruction()
    est.FilterInitialViewGraphAndCalibrateCameras(vg, scene)
    est.orientations = o
    keys, keep = flat_marks(vg, o, 48, 0.02, 1)
    expected_edges = {k for k, kp in zip(keys, keep) if kp}
    comps = components(expected_edges)
    big = comps[0]
    expected_edges = {k for k in expected_edges if k[0] in big and k[1] in big}
    est.FilterRelativeTranslation()
    assert set(vg.GetAllEdges().keys()) == expected_edges
    assert set(int(v) for v in vg.ViewIds()) == big
    assert set(int(v) for v in est.orientations.keys()) == big
    print("estimator: %d of %d edges kept by the filter, %d views of %d in the largest component" % (int(keep.sum()), keep.size, len(big), 150))


def test_yaml_switch_off_leaves_the_graph_unchanged(tmp_path):
    sfm = _sfm()
    g, ids, vg, o = estimator_graph(sfm)
    flags = tmp_path / "flags.yaml"
    flags.write_text("num_threads: 2\nfilter_relative_translations_with_1dsfm: false\n")
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts)
    assert opts.reconstruction_estimator_options.filter_relative_translations_with_1dsfm is False
    est = sfm.GlobalReconstructionEstimator(opts.reconstruction_estimator_options)
    est.FilterInitialViewGraphAndCalibrateCameras(vg, sfm.Reconstruction())
    est.orientations = o
    before = set(vg.GetAllEdges().keys())
    est.FilterRelativeTranslation()
    assert set(vg.GetAllEdges().keys()) == before and len(est.orientations) == 150
    flags.write_text("filter_relative_translations_with_1dsfm: true\n")
    opts2 = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(flags), opts2)
    assert opts2.reconstruction_estimator_options.filter_relative_translations_with_1dsfm is True
