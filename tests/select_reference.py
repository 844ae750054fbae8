"""An independent restatement of steps 2 and 3 of gsfm_tracks_select_good (include/gsfm_tracks.h), given the statistics (n, mean) per track:
dicts and sorted lists, following the header text.  It shares no code with the C++."""
import struct

import numpy as np

COUNT_NAMES = ("tracks_with_items", "cells", "selected_by_cell", "cameras_topped_up", "selected_by_top_up", "selected")
NAN_BITS = 0x7ff8000000000000


def mean_bits(mean):
    """The mean as the header compares it: its bit pattern as an unsigned 64-bit integer, every NaN replaced by one pattern."""
    mean = float(mean)
    if mean != mean:
        return NAN_BITS
    return struct.unpack("<Q", struct.pack("<d", mean))[0]


def cell_of(x, cell_size):
    """(int32) trunc(x * (1.0 / S)): one multiplication, truncation toward zero."""
    return int(float(x) * (1.0 / float(cell_size)))


def select(n_cams, track_ptr, obs_cam, obs_xy, n_views, mean_sq_err, cam_estimated=None, point_estimated=None, long_track_length_threshold=10,
           image_grid_cell_size_pixels=100, min_num_optimized_tracks_per_view=200):
    """Returns (selected: uint8 per track, counts: dict of COUNT_NAMES)."""
    L, S, K = int(long_track_length_threshold), int(image_grid_cell_size_pixels), int(min_num_optimized_tracks_per_view)
    tp = [int(v) for v in track_ptr]
    T = len(tp) - 1
    xy = np.asarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    cam_ok = [True] * n_cams if cam_estimated is None else [bool(v) for v in cam_estimated]
    trk_ok = [True] * T if point_estimated is None else [bool(v) for v in point_estimated]
    # the items: (camera, track, place), an observation of an estimated track in an estimated camera
    items = [(int(obs_cam[o]), t, o - tp[t]) for t in range(T) if trk_ok[t] for o in range(tp[t], tp[t + 1]) if cam_ok[int(obs_cam[o])]]
    key = {t: (min(int(n_views[t]), L), mean_bits(mean_sq_err[t]), t) for t in range(T) if trk_ok[t]}
    selected = np.zeros(T, dtype=np.uint8)
    # step 2: per non-empty cell the smallest (key, track index)
    best = {}
    for cam, t, place in items:
        o = tp[t] + place
        cell = (cam, cell_of(xy[o, 0], S), cell_of(xy[o, 1], S))
        if cell not in best or key[t] < best[cell]:
            best[cell] = key[t]
    for k in best.values():
        selected[k[2]] = 1
    by_cell = int(np.count_nonzero(selected == 1))
    # step 3: the cameras in ascending index, each over its items by ascending (track, place)
    per_cam = {}
    for it in sorted(items):
        per_cam.setdefault(it[0], []).append(it)
    topped, added = 0, 0
    for cam in sorted(per_cam):
        mine = per_cam[cam]
        est = len(mine)
        opt = sum(1 for _, t, _ in mine if selected[t])
        if K == 0 or opt >= K or opt == est:
            continue
        m = min(K - opt, est - opt)
        free = [t for _, t, _ in mine if not selected[t]][:m]   # not selected as this camera's turn begins
        for t in free:
            if not selected[t]:
                selected[t] = 2
                added += 1
        topped += 1
    counts = dict(zip(COUNT_NAMES, (sum(1 for t in range(T) if trk_ok[t] and int(n_views[t]) >= 1), len(best), by_cell, topped, added, by_cell + added)))
    return selected, counts
