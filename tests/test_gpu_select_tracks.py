"""-m gpu: gsfm_tracks_select_good on the device (include/gsfm_tracks.h) against the outlier rule's statistics, the restatement
tests/select_reference.py and the sequential host entry, on one synthetic scene: 12 cameras (one unestimated), about 300 tracks of every lane
class (lengths up to 70 over 12 cameras, so the long tracks list cameras more than once), some unestimated, 0.7 px of pixel noise and perturbed
points so that the means differ, a handful of tracks duplicated exactly so that equal keys occur, some coordinates on exact multiples of the
cell sizes and some negative."""
import numpy as np
import pytest

from globalsfmpy_amd import solver, synth

import select_reference as ref

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 5, 8, 9, 20, 64, 65, 70)
UNESTIMATED_CAMERA = 5
GRID = [(S, K, L) for S in (1, 7, 100) for K in (0, 3, 1000) for L in (1, 10)]
MAIN = (300, 400, 10)   # S, K, L of the setting whose selection must be a proper subset


def raw(x):
    return np.ascontiguousarray(x).view(np.uint8)


def build(seed, n_tracks, duplicates):
    s = synth.make_tracks(12, n_tracks, seed, lengths=LENGTHS, noise_px=0.7)
    rng = np.random.default_rng(seed + 1000)
    ptr, cam, xy = s["track_ptr"].astype(np.int64), s["obs_cam"], s["obs_xy"].copy()
    points = s["gt_points"] + 0.01 * rng.standard_normal(s["gt_points"].shape)
    n_obs = xy.shape[0]
    on_grid = rng.choice(n_obs, 60, replace=False)                    # exact multiples of 100 (and so of 1; of 7 where 7 divides them)
    xy[on_grid, 0] = np.round(xy[on_grid, 0] / 100.0) * 100.0
    xy[on_grid[:20], 1] = np.round(xy[on_grid[:20], 1] / 700.0) * 700.0
    negative = rng.choice(n_obs, 60, replace=False)
    xy[negative] -= np.array([1300.0, 900.0])
    xy[negative[:10], 0] = -100.0                                      # on a cell edge left of zero
    xy[negative[10:20], 0] = -0.5                                      # shares cell 0 with the small positive coordinates
    tracks = [(cam[ptr[t]:ptr[t + 1]], xy[ptr[t]:ptr[t + 1]], points[t]) for t in range(n_tracks)]
    for t in rng.choice(n_tracks, duplicates, replace=False):          # exact copies, appended: same observations, same point, same key
        tracks.append(tracks[int(t)])
    order = rng.permutation(len(tracks))                               # (so that a copy does not always have the larger index)
    tracks = [tracks[int(k)] for k in order]
    T = len(tracks)
    cam_estimated = np.ones(12, np.uint8)
    cam_estimated[UNESTIMATED_CAMERA] = 0
    point_estimated = np.ones(T, np.uint8)
    point_estimated[rng.choice(T, T // 10, replace=False)] = 0
    return dict(rot_aa=s["rot_aa"], cam_pos=s["cam_pos"], intrinsics=s["intrinsics"], cam_estimated=cam_estimated, point_estimated=point_estimated,
                track_ptr=np.concatenate([[0], np.cumsum([len(c) for c, _, _ in tracks])]).astype(np.uint64),
                obs_cam=np.concatenate([c for c, _, _ in tracks]).astype(np.uint32), obs_xy=np.concatenate([p for _, p, _ in tracks]),
                points=np.array([x for _, _, x in tracks]))


def run(b, S=100, K=200, L=10, capacity=0, **over):
    a = dict(b, **over)
    return solver.select_good_tracks(a["rot_aa"], a["cam_pos"], a["intrinsics"], a["track_ptr"], a["obs_cam"], a["obs_xy"], a["points"],
                                     cam_estimated=a["cam_estimated"], point_estimated=a["point_estimated"], long_track_length_threshold=L,
                                     image_grid_cell_size_pixels=S, min_num_optimized_tracks_per_view=K, hash_capacity_log2=capacity)


def restated(b, stats, S, K, L):
    return ref.select(12, b["track_ptr"], b["obs_cam"], b["obs_xy"], stats["n_views"], stats["mean_sq_err"], cam_estimated=b["cam_estimated"],
                      point_estimated=b["point_estimated"], long_track_length_threshold=L, image_grid_cell_size_pixels=S, min_num_optimized_tracks_per_view=K)


def n_items(b):
    track_of = np.repeat(np.arange(len(b["track_ptr"]) - 1), np.diff(b["track_ptr"].astype(np.int64)))
    return int(np.count_nonzero((b["cam_estimated"][b["obs_cam"]] != 0) & (b["point_estimated"][track_of] != 0)))


@pytest.fixture(scope="module")
def batch():
    return build(31, 300, 8)


@pytest.fixture(scope="module")
def main(batch):
    return run(batch, *MAIN[:2], MAIN[2])


def test_the_scene_holds_what_the_tests_need(batch):
    lens = np.diff(batch["track_ptr"].astype(np.int64))
    assert (lens <= 8).any() and ((lens >= 9) & (lens <= 64)).any() and (lens >= 65).any()       # every lane class
    assert (batch["point_estimated"] == 0).sum() >= 10 and batch["cam_estimated"].sum() == 11
    xy = batch["obs_xy"]
    assert (xy[:, 0] % 100.0 == 0.0).sum() >= 40 and (xy < 0).any(axis=1).sum() >= 40 and (xy[:, 0] == -0.5).sum() == 10


def test_statistics_equal_the_outlier_rule_s_bit_for_bit(batch, main):
    out = solver.outlier_tracks(batch["rot_aa"], batch["cam_pos"], batch["intrinsics"], batch["track_ptr"], batch["obs_cam"], batch["obs_xy"],
                                batch["points"], cam_estimated=batch["cam_estimated"], point_estimated=batch["point_estimated"])
    assert np.array_equal(main["n_views"], out["n_views"])
    assert np.array_equal(raw(main["mean_sq_err"]), raw(out["mean_sq_err"]))
    off = batch["point_estimated"] == 0
    assert not main["n_views"][off].any() and not raw(main["mean_sq_err"][off]).any() and not main["selected"][off].any()
    est = ~off
    assert len(np.unique(main["mean_sq_err"][est])) < est.sum()          # the duplicated tracks: equal means occur
    assert len(np.unique(main["mean_sq_err"][est])) > 0.9 * est.sum()    # ... and the means differ otherwise
    assert main["kernel_ms"] > 0


def test_the_main_setting_selects_a_proper_subset(batch, main):
    want, want_counts = restated(batch, main, *MAIN)
    print("main setting S, K, L = %s: %s; %d items downloaded for the top-up" % (MAIN, want_counts, main["deficient_items"]))
    assert 0 < want_counts["selected"] < want_counts["tracks_with_items"] <= int(batch["point_estimated"].sum())
    assert want_counts["selected_by_cell"] > 0 and want_counts["selected_by_top_up"] > 0 and 0 < want_counts["cameras_topped_up"] <= 11
    assert main["counts"] == want_counts and np.array_equal(main["selected"], want)
    assert set(np.unique(main["selected"])) == {0, 1, 2}


@pytest.mark.parametrize("S,K,L", GRID)
def test_selection_and_counts_equal_the_restatement_and_the_sequential_entry(batch, S, K, L):
    dev = run(batch, S, K, L)
    want, want_counts = restated(batch, dev, S, K, L)
    seq = solver.select_good_tracks_from_statistics(12, batch["track_ptr"], batch["obs_cam"], batch["obs_xy"], dev["n_views"], dev["mean_sq_err"],
                                                    cam_estimated=batch["cam_estimated"], point_estimated=batch["point_estimated"],
                                                    long_track_length_threshold=L, image_grid_cell_size_pixels=S, min_num_optimized_tracks_per_view=K)
    print("S %d K %d L %d: %s, %d deficient items" % (S, K, L, dev["counts"], dev["deficient_items"]))
    assert dev["counts"] == want_counts == seq["counts"]
    assert np.array_equal(dev["selected"], want) and np.array_equal(seq["selected"], want)
    if K == 0:         # no camera is deficient
        assert want_counts["cameras_topped_up"] == 0 and dev["deficient_items"] == 0 and not (want == 2).any()
    if K == 1000:      # every camera that is not complete after step 2 is deficient, and ends complete
        assert want_counts["selected"] == want_counts["tracks_with_items"]
        if S == 100:
            assert want_counts["cameras_topped_up"] >= 1 and dev["deficient_items"] > 0


def test_every_camera_deficient_and_none(batch):
    all_deficient = run(batch, 2000, 1000, 10)    # one or two cells per camera and a minimum no camera reaches: every estimated camera tops up ...
    assert all_deficient["deficient_items"] == n_items(batch)             # ... so every item is downloaded
    want, want_counts = restated(batch, all_deficient, 2000, 1000, 10)
    assert all_deficient["counts"] == want_counts and np.array_equal(all_deficient["selected"], want)
    assert want_counts["cameras_topped_up"] >= 1 and want_counts["selected"] == want_counts["tracks_with_items"]
    none = run(batch, 1, 1, 10)                   # cells of one pixel: every camera holds a selected track at once
    assert none["deficient_items"] == 0 and none["counts"]["cameras_topped_up"] == 0


@pytest.mark.parametrize("S,K,L", [MAIN, (7, 3, 1), (1, 1000, 10)])
def test_the_smallest_table_returns_the_same_bytes(batch, S, K, L):
    smallest = max(1, int(np.ceil(np.log2(n_items(batch)))))
    a, b = run(batch, S, K, L), run(batch, S, K, L, capacity=smallest)
    assert a["counts"] == b["counts"] and all(np.array_equal(raw(a[k]), raw(b[k])) for k in ("selected", "n_views", "mean_sq_err"))
    with pytest.raises(solver.SolverError, match="fewer slots"):
        run(batch, S, K, L, capacity=smallest - 1)


def test_two_calls_return_the_same_bytes(batch, main):
    again = run(batch, *MAIN[:2], MAIN[2])
    assert again["counts"] == main["counts"] and all(np.array_equal(raw(again[k]), raw(main[k])) for k in ("selected", "n_views", "mean_sq_err"))


def test_permuting_the_tracks_permutes_statistics_and_cell_winners():
    b = build(32, 120, 0)                          # no duplicated tracks: no two tracks share a key, so the index decides nothing
    T = len(b["track_ptr"]) - 1
    perm = np.random.default_rng(5).permutation(T)   # the new track k is the old track perm[k]
    ptr = b["track_ptr"].astype(np.int64)
    p = dict(b, track_ptr=np.concatenate([[0], np.cumsum(np.diff(ptr)[perm])]).astype(np.uint64),
             obs_cam=np.concatenate([b["obs_cam"][ptr[t]:ptr[t + 1]] for t in perm]), obs_xy=np.concatenate([b["obs_xy"][ptr[t]:ptr[t + 1]] for t in perm]),
             points=b["points"][perm], point_estimated=b["point_estimated"][perm])
    for S, L in ((100, 10), (7, 1), (600, 3)):
        x, y = run(b, S, 0, L), run(p, S, 0, L)
        est = b["point_estimated"] != 0
        assert len(np.unique(x["mean_sq_err"][est].view(np.uint64))) == est.sum()      # no two tracks share a mean, so none share a key
        assert np.array_equal(y["n_views"], x["n_views"][perm]) and np.array_equal(raw(y["mean_sq_err"]), raw(x["mean_sq_err"][perm]))
        assert np.array_equal(y["selected"] == 1, (x["selected"] == 1)[perm])
        assert 0 < (x["selected"] == 1).sum() and y["counts"] == x["counts"]
        if S == 600:   # a handful of cells per camera: the winners are a proper subset, so the check above can fail
            assert (x["selected"] == 1).sum() < est.sum()


def test_another_track_s_flag_changes_nothing_for_this_one(batch, main):
    pe = batch["point_estimated"].copy()
    pe[np.flatnonzero(pe)[::3]] = 0
    fewer = run(batch, *MAIN[:2], MAIN[2], point_estimated=pe)
    still = pe != 0
    assert np.array_equal(fewer["n_views"][still], main["n_views"][still]) and np.array_equal(raw(fewer["mean_sq_err"][still]), raw(main["mean_sq_err"][still]))
    assert not fewer["selected"][~still].any() and not fewer["n_views"][~still].any()
