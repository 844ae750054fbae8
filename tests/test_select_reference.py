"""Hand-made cases on the restatement of the track selection alone (tests/select_reference.py): they pin the literal rules of
include/gsfm_tracks.h, gsfm_tracks_select_good -- the shorter truncated length wins a cell, equal keys go to the lower index, NaN loses to
+inf, truncation toward zero, and the top-up by track index."""
import numpy as np

import select_reference as ref

INF, NAN = float("inf"), float("nan")


def scene(tracks, n_cams=None):
    """tracks: per track a list of (camera, x, y).  Returns (n_cams, track_ptr, obs_cam, obs_xy)."""
    ptr, cam, xy = [0], [], []
    for obs in tracks:
        for c, x, y in obs:
            cam.append(c)
            xy.append((x, y))
        ptr.append(len(cam))
    n = max(cam) + 1 if n_cams is None else n_cams
    return n, np.array(ptr, np.uint64), np.array(cam, np.uint32), np.array(xy, np.float64).reshape(-1, 2)


def run(tracks, n, mean, **kw):
    kw.setdefault("min_num_optimized_tracks_per_view", 0)
    return ref.select(*scene(tracks), n, mean, **kw)


def test_the_shorter_truncated_length_wins_the_cell():
    sel, counts = run([[(0, 10.0, 10.0)], [(0, 20.0, 20.0)]], [3, 12], [4.0, 0.1], long_track_length_threshold=10)
    assert sel.tolist() == [1, 0] and counts["cells"] == 1 and counts["selected_by_cell"] == 1


def test_lengths_at_or_above_the_threshold_tie_and_the_error_decides():
    sel, _ = run([[(0, 10.0, 10.0)], [(0, 20.0, 20.0)]], [10, 12], [4.0, 0.1], long_track_length_threshold=10)
    assert sel.tolist() == [0, 1]


def test_equal_keys_go_to_the_lower_index():
    sel, _ = run([[(0, 90.0, 10.0)], [(0, 20.0, 20.0)], [(0, 30.0, 5.0)]], [4, 4, 4], [2.5, 2.5, 2.5])
    assert sel.tolist() == [1, 0, 0]


def test_a_nan_mean_loses_to_infinity_and_infinity_to_every_finite_mean():
    assert run([[(0, 1.0, 1.0)], [(0, 2.0, 2.0)]], [2, 2], [NAN, INF])[0].tolist() == [0, 1]
    assert run([[(0, 1.0, 1.0)], [(0, 2.0, 2.0)]], [2, 2], [INF, 1e300])[0].tolist() == [0, 1]
    assert ref.mean_bits(-NAN) == ref.mean_bits(NAN) == ref.NAN_BITS > ref.mean_bits(INF) > ref.mean_bits(1.7e308) > ref.mean_bits(0.0) == 0


def test_cells_truncate_toward_zero():
    assert ref.cell_of(-0.5, 100) == 0 and ref.cell_of(-100.5, 100) == -1 and ref.cell_of(300.0, 100) == 3
    assert ref.cell_of(99.999, 100) == 0 and ref.cell_of(-99.999, 100) == 0 and ref.cell_of(-100.0, 100) == -1
    # x = -0.5 shares cell 0 with x = 0.5; x = -100.5 does not; x = 300 lies with 399, not with 299
    sel, counts = run([[(0, -0.5, 0.0)], [(0, 0.5, 0.0)], [(0, -100.5, 0.0)], [(0, 300.0, 0.0)], [(0, 399.0, 0.0)], [(0, 299.0, 0.0)]], [2] * 6,
                      [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], image_grid_cell_size_pixels=100)
    assert sel.tolist() == [1, 0, 1, 1, 0, 1] and counts["cells"] == 4


def test_the_top_up_takes_the_lowest_track_indices_whatever_their_errors():
    # one cell in one camera: track 3 (the best) wins it; K = 3 adds the tracks 0 and 1, whose errors are the worst
    tracks = [[(0, 10.0 + k, 10.0)] for k in range(5)]
    sel, counts = run(tracks, [2] * 5, [9.0, 8.0, 1.0, 0.5, 0.7], min_num_optimized_tracks_per_view=3)
    assert sel.tolist() == [2, 2, 0, 1, 0]
    assert counts == dict(zip(ref.COUNT_NAMES, (5, 1, 1, 1, 2, 3)))


def test_a_chained_top_up_counts_what_earlier_cameras_added():
    # one cell per camera; track 0 is the best everywhere and wins both cells.  Camera 0 sees the tracks 0, 1, 2, camera 1 sees all five.
    tracks = [[(0, 10.0, 10.0), (1, 10.0, 10.0)] for _ in range(3)] + [[(1, 10.0, 10.0)] for _ in range(2)]
    n, ptr, cam, xy = scene(tracks)
    nv, mean = [2, 2, 2, 1, 1], [1.0, 2.0, 3.0, 4.0, 5.0]
    # K = 4.  Camera 0: est 3, opt 1, m = min(3, 2) = 2: it adds 1 and 2.  Camera 1 then holds 0, 1, 2: opt 3, m = min(1, 2) = 1: it adds 3 alone.
    sel, counts = ref.select(n, ptr, cam, xy, nv, mean, long_track_length_threshold=1, min_num_optimized_tracks_per_view=4)
    assert sel.tolist() == [1, 2, 2, 2, 0] and counts["cameras_topped_up"] == 2 and counts["selected_by_top_up"] == 3
    # without camera 0 camera 1 starts from opt 1 and adds three tracks itself
    alone, c1 = ref.select(n, ptr, cam, xy, [1] * 5, mean, cam_estimated=[0, 1], long_track_length_threshold=1, min_num_optimized_tracks_per_view=4)
    assert alone.tolist() == [1, 2, 2, 2, 0] and c1["cameras_topped_up"] == 1 and c1["selected_by_top_up"] == 3
    # K = 3: camera 0's two additions meet camera 1's minimum, which adds nothing
    sel3, c3 = ref.select(n, ptr, cam, xy, nv, mean, long_track_length_threshold=1, min_num_optimized_tracks_per_view=3)
    assert sel3.tolist() == [1, 2, 2, 0, 0] and c3["cameras_topped_up"] == 1


def test_k_zero_adds_nothing():
    tracks = [[(0, 10.0 + k, 10.0)] for k in range(4)]
    sel, counts = run(tracks, [2] * 4, [1.0, 2.0, 3.0, 4.0], min_num_optimized_tracks_per_view=0)
    assert sel.tolist() == [1, 0, 0, 0] and counts["cameras_topped_up"] == 0 and counts["selected_by_top_up"] == 0


def test_a_camera_whose_every_item_is_selected_adds_nothing():
    tracks = [[(0, 10.0, 10.0)], [(0, 210.0, 10.0)]]   # two cells, both tracks selected: opt = est = 2 < K
    sel, counts = run(tracks, [2, 2], [1.0, 2.0], min_num_optimized_tracks_per_view=100)
    assert sel.tolist() == [1, 1] and counts["cameras_topped_up"] == 0


def test_tracks_and_cameras_that_are_not_estimated_hold_no_item():
    tracks = [[(0, 10.0, 10.0), (1, 10.0, 10.0)], [(0, 20.0, 10.0), (1, 20.0, 10.0)], [(1, 30.0, 10.0)]]
    n, ptr, cam, xy = scene(tracks)
    sel, counts = ref.select(n, ptr, cam, xy, [1, 0, 0], [5.0, 0.1, 0.1], cam_estimated=[1, 0], point_estimated=[1, 0, 1], min_num_optimized_tracks_per_view=9)
    assert sel.tolist() == [1, 0, 0] and counts == dict(zip(ref.COUNT_NAMES, (1, 1, 1, 0, 0, 1)))
