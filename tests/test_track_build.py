"""gsfm_tracks_build_sequential (the C++ sequential restatement of include/gsfm_tracks.h's track builder, host code: no device) against the
pure-Python restatement of tests/track_build_reference.py, exactly; and the argument errors both entries share."""
import numpy as np
import pytest

import track_build_reference as ref
from globalsfmpy_amd import solver

CASES = ref.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_sequential_equals_python_restatement(name):
    case = CASES[name]
    want = ref.build_tracks_reference(**ref.call_arguments(case))
    for key, value in case["expect"].items():   # the case is what its name says
        assert want["counts"][key] == value, (key, want["counts"])
    got = solver.build_tracks(hash_capacity_log2=case["hash_capacity_log2"], sequential=True, **ref.call_arguments(case))
    ref.assert_same_tracks(got, want)
    assert got["kernel_ms"] == 0.0


def test_sequential_same_bytes_twice():
    case = CASES["random_mix_max_5"]
    a = solver.build_tracks(sequential=True, **ref.call_arguments(case))
    b = solver.build_tracks(sequential=True, **ref.call_arguments(case))
    ref.assert_same_tracks(a, b)


def test_negative_zero_keeps_the_first_pixel_bits():
    got = solver.build_tracks(sequential=True, **ref.call_arguments(CASES["negative_zero"]))
    assert np.signbit(got["obs_xy"][0, 0]) and got["obs_xy"][0, 0] == 0.0


@pytest.mark.parametrize("sequential", [True, False])
def test_argument_errors(sequential):
    """refused on the host before any device call: the device entry reports them without a device"""
    args = ref.call_arguments(ref.non_finite_case())
    with pytest.raises(solver.SolverError, match="not finite"):
        solver.build_tracks(sequential=sequential, **args)
    with pytest.raises(ValueError):
        ref.build_tracks_reference(**args)
    args = ref.call_arguments(CASES["random_mix"])
    with pytest.raises(solver.SolverError, match="fewer slots"):   # 240 matches, 480 endpoints: 2^8 slots are too few
        solver.build_tracks(hash_capacity_log2=8, sequential=sequential, **args)
    with pytest.raises(solver.SolverError, match="at least 1"):
        solver.build_tracks(sequential=sequential, **dict(args, min_track_length=0))
    with pytest.raises(solver.SolverError, match="view"):
        solver.build_tracks(sequential=sequential, **dict(args, n_views=5))
    same = dict(args, edge_j=args["edge_i"])
    with pytest.raises(solver.SolverError, match="itself"):
        solver.build_tracks(sequential=sequential, **same)
    bad_ptr = args["match_ptr"].copy()
    bad_ptr[1], bad_ptr[2] = bad_ptr[2] + 1, bad_ptr[1]
    if bad_ptr[2] < bad_ptr[1]:
        with pytest.raises(solver.SolverError, match="decreases"):
            solver.build_tracks(sequential=sequential, **dict(args, match_ptr=bad_ptr))


def test_check_view_builds_the_tracks_of_the_colmap_branch(tmp_path):
    """The host half of the end-to-end test (tests/test_gpu_track_build.py runs the pipeline on): after the COLMAP ingestion CheckView() builds
    the tracks from the matches.  With a device NumTracks() is the restatement's; without one nothing can build them, and CheckView() says so
    and leaves the reconstruction without tracks, as the ingestion left it."""
    import warnings
    sfm = ref.sfm_module()
    wildcard = ref.write_colmap_scene(str(tmp_path))
    opts = sfm.ReconstructionBuilderOptions()
    sfm.load_1DSFM_config(str(tmp_path / "flags.yaml"), opts)
    assert opts.min_track_length == 2 and opts.max_track_length == 1000
    builder = sfm.ReconstructionBuilder(opts, sfm.FeaturesAndMatchesDatabase(str(tmp_path / "database")))
    sfm.AddColmapMatchesToReconstructionBuilder(str(tmp_path / "two_views.txt"), wildcard, builder)
    rec = builder.get_reconstruction()
    assert rec.NumTracks() == 0 and rec.LastTrackBuildSummary() is None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        builder.CheckView()
    summary = rec.LastTrackBuildSummary()
    want, _ = ref.reference_of_reconstruction(rec)
    assert want["counts"]["tracks"] >= 140
    if summary["built"]:
        assert not caught
        assert rec.NumTracks() == want["counts"]["tracks"] == summary["tracks"]
        assert {k: summary[k] for k in ref.COUNT_NAMES} == want["counts"]
    else:
        assert "no HIP device" in summary["error"] and rec.NumTracks() == 0
        assert any("no tracks were built" in str(w.message) for w in caught)
