"""gsfm_tracks_select_good_from_statistics (sequential host code, no device) against the restatement tests/select_reference.py on random
scenes: 8 cameras, 200 tracks of 2 to 70 observations, some cameras and tracks unestimated, statistics drawn with ties, inf and NaN."""
import numpy as np
import pytest

from globalsfmpy_amd import solver

import select_reference as ref

N_CAMS, N_TRACKS = 8, 200


def make_scene(seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(2, 71, N_TRACKS)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    n_obs = int(ptr[-1])
    obs_cam = rng.integers(0, N_CAMS, n_obs).astype(np.uint32)          # (a track may list a camera more than once: each is an item)
    obs_xy = rng.uniform(-150.0, 650.0, (n_obs, 2))
    on_grid = rng.random(n_obs) < 0.1                                   # some coordinates on exact multiples of the cell sizes
    obs_xy[on_grid] = np.round(obs_xy[on_grid] / 100.0) * 100.0
    cam_estimated = np.ones(N_CAMS, np.uint8)
    cam_estimated[rng.choice(N_CAMS, 2, replace=False)] = 0
    point_estimated = (rng.random(N_TRACKS) < 0.85).astype(np.uint8)
    n_views = np.array([int(np.count_nonzero(cam_estimated[obs_cam[int(ptr[t]):int(ptr[t + 1])]])) for t in range(N_TRACKS)], np.int32)
    mean = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, 7.5], N_TRACKS) + np.where(rng.random(N_TRACKS) < 0.5, 0.0, rng.random(N_TRACKS))   # deliberate ties
    mean[rng.choice(N_TRACKS, 12, replace=False)] = np.inf
    mean[rng.choice(N_TRACKS, 12, replace=False)] = np.nan
    mean[rng.choice(N_TRACKS, 3, replace=False)] = -np.nan              # a NaN of the other sign is the same key
    return dict(n_cams=N_CAMS, track_ptr=ptr, obs_cam=obs_cam, obs_xy=obs_xy, cam_estimated=cam_estimated, point_estimated=point_estimated,
                n_views=n_views, mean_sq_err=mean)


@pytest.fixture(scope="module", params=[11, 12])
def scene(request):
    return make_scene(request.param)


@pytest.mark.parametrize("L", [1, 10])
@pytest.mark.parametrize("K", [0, 3, 1000])
@pytest.mark.parametrize("S", [1, 7, 100])
def test_flags_and_counts_equal_the_restatement(scene, S, K, L):
    kw = dict(long_track_length_threshold=L, image_grid_cell_size_pixels=S, min_num_optimized_tracks_per_view=K)
    want, want_counts = ref.select(scene["n_cams"], scene["track_ptr"], scene["obs_cam"], scene["obs_xy"], scene["n_views"], scene["mean_sq_err"],
                                   cam_estimated=scene["cam_estimated"], point_estimated=scene["point_estimated"], **kw)
    got = solver.select_good_tracks_from_statistics(scene["n_cams"], scene["track_ptr"], scene["obs_cam"], scene["obs_xy"], scene["n_views"],
                                                    scene["mean_sq_err"], cam_estimated=scene["cam_estimated"], point_estimated=scene["point_estimated"], **kw)
    assert got["counts"] == want_counts
    assert np.array_equal(got["selected"], want)
    assert not got["selected"][scene["point_estimated"] == 0].any()
    if K == 0:
        assert not (want == 2).any()
    if K == 1000:   # every camera is deficient until all its items are selected: every track with an item ends up selected
        assert want_counts["selected"] == want_counts["tracks_with_items"]


def test_no_flags_means_everything_is_estimated(scene):
    nv = np.diff(scene["track_ptr"].astype(np.int64)).astype(np.int32)
    want, want_counts = ref.select(scene["n_cams"], scene["track_ptr"], scene["obs_cam"], scene["obs_xy"], nv, scene["mean_sq_err"],
                                   image_grid_cell_size_pixels=400, min_num_optimized_tracks_per_view=40)
    got = solver.select_good_tracks_from_statistics(scene["n_cams"], scene["track_ptr"], scene["obs_cam"], scene["obs_xy"], nv, scene["mean_sq_err"],
                                                    image_grid_cell_size_pixels=400, min_num_optimized_tracks_per_view=40)
    assert got["counts"] == want_counts and np.array_equal(got["selected"], want)
    assert 0 < want_counts["selected"] < N_TRACKS and want_counts["selected_by_top_up"] > 0
