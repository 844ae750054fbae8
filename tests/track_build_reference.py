"""A small pure-Python restatement of Theia's TrackBuilder under the definition of include/gsfm_tracks.h (gsfm_tracks_build), written
independently of the C++ one: dicts for the features, the sequential union rule of connected_components.h:87-108 over ALL matches (no
split into plain components and a replay), then BuildTracks.  Also the test cases both track-building test files run."""
import math

import numpy as np

COUNT_NAMES = ("features", "components", "small", "inconsistent", "degenerate", "replayed", "tracks")


def build_tracks_reference(n_views, edge_i, edge_j, match_ptr, matches, min_track_length=2, max_track_length=1000):
    matches = np.asarray(matches, dtype=np.float64).reshape(-1, 4)
    feature_id = {}          # (view, x, y) -> id; Python's float equality and hash make -0.0 and 0.0 one key
    feature = []             # id -> (view, x, y) of the first endpoint met
    pairs = []
    for e in range(len(edge_i)):
        for m in range(int(match_ptr[e]), int(match_ptr[e + 1])):
            ids = []
            for view, x, y in ((int(edge_i[e]), matches[m, 0], matches[m, 1]), (int(edge_j[e]), matches[m, 2], matches[m, 3])):
                if not (math.isfinite(x) and math.isfinite(y)):
                    raise ValueError("match %d has a coordinate that is not finite" % m)
                key = (view, float(x), float(y))
                if key not in feature_id:
                    feature_id[key] = len(feature)
                    feature.append(key)
                ids.append(feature_id[key])
            pairs.append(tuple(ids))

    def components(limit):
        root, size = {}, {}

        def find(a):
            while root[a] != a:
                a = root[a]
            return a
        for f in range(len(feature)):
            root[f], size[f] = f, 1
        for a, b in pairs:
            ra, rb = find(a), find(b)
            if ra == rb or (limit is not None and size[ra] + size[rb] > limit):
                continue
            if size[ra] < size[rb]:
                ra, rb = rb, ra
            root[rb] = ra
            size[ra] += size[rb]
        groups = {}
        for f in range(len(feature)):      # ascending f: a group's first member is its smallest id, its members are in ascending id
            groups.setdefault(find(f), []).append(f)
        return sorted(groups.values(), key=lambda g: g[0])

    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["features"] = len(feature)
    counts["replayed"] = sum(1 for g in components(None) if len(g) > max_track_length)
    track_ptr, obs_view, obs_xy = [0], [], []
    for group in components(max_track_length):
        counts["components"] += 1
        if len(group) < min_track_length:
            counts["small"] += 1
            continue
        seen, kept = set(), []
        for f in group:
            if feature[f][0] in seen:
                counts["inconsistent"] += 1
                continue
            seen.add(feature[f][0])
            kept.append(f)
        if len(kept) < 2:
            counts["degenerate"] += 1
            continue
        for f in kept:
            obs_view.append(feature[f][0])
            obs_xy.append(feature[f][1:])
        track_ptr.append(len(obs_view))
    counts["tracks"] = len(track_ptr) - 1
    return {"track_ptr": np.array(track_ptr, dtype=np.uint64), "obs_view": np.array(obs_view, dtype=np.uint32),
            "obs_xy": np.array(obs_xy, dtype=np.float64).reshape(-1, 2), "counts": counts}


def assert_same_tracks(got, want):
    """Exactly: the same track_ptr, views, pixel BITS (so -0.0 is not 0.0 here) and counts."""
    assert got["counts"] == want["counts"]
    assert np.array_equal(got["track_ptr"], want["track_ptr"])
    assert np.array_equal(got["obs_view"], want["obs_view"])
    assert got["obs_xy"].shape == want["obs_xy"].shape
    assert np.array_equal(np.ascontiguousarray(got["obs_xy"]).view(np.uint64), np.ascontiguousarray(want["obs_xy"]).view(np.uint64))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _flatten(n_views, calls, **options):
    """calls: (view_a, (x, y), view_b, (x, y)) in call order, or (view_a, view_b) alone for an edge without matches.  Consecutive calls of
    one view pair make one edge, so the call order is the flattened order."""
    edge_i, edge_j, match_ptr, rows = [], [], [0], []
    for call in calls:
        a, b = (call[0], call[2]) if len(call) == 4 else call
        if not edge_i or (edge_i[-1], edge_j[-1]) != (a, b) or len(call) == 2:
            edge_i.append(a); edge_j.append(b); match_ptr.append(match_ptr[-1])
        if len(call) == 4:
            rows.append(call[1] + call[3])
            match_ptr[-1] += 1
    case = {"n_views": n_views, "edge_i": np.array(edge_i, dtype=np.uint32), "edge_j": np.array(edge_j, dtype=np.uint32),
            "match_ptr": np.array(match_ptr, dtype=np.uint64), "matches": np.array(rows, dtype=np.float64).reshape(-1, 4),
            "min_track_length": 2, "max_track_length": 1000, "hash_capacity_log2": 0, "expect": {}}
    case.update(options)
    return case


def _pix(view, k):
    return (100.0 + view + 0.25 * k, 50.0 + 3.0 * k)


def _path(views, order, k=0):
    """matches joining consecutive views' features, listed in `order` (a permutation of the links)"""
    return [(views[j], _pix(views[j], k), views[j + 1], _pix(views[j + 1], k)) for j in order]


def _scrambled(n_links, seed):
    return [int(j) for j in np.random.RandomState(seed).permutation(n_links)]


def min_capacity_log2(n_matches):
    k = 0
    while (1 << k) < 2 * n_matches:
        k += 1
    return k


def cases():
    out = {}
    p, q, r, s = (10.5, 20.25), (11.0, 21.0), (12.0, 22.0), (13.0, 23.0)
    out["shared_by_three_edges"] = _flatten(4, [(0, p, 1, q), (0, p, 2, r), (0, p, 3, s)], expect={"features": 4, "tracks": 1})
    out["same_pixel_two_views"] = _flatten(3, [(0, p, 1, p), (1, p, 2, r)], expect={"features": 3, "tracks": 1})
    out["negative_zero"] = _flatten(3, [(0, (-0.0, 5.0), 1, q), (0, (0.0, 5.0), 2, r)], expect={"features": 3, "tracks": 1})
    out["equal_x_other_y"] = _flatten(3, [(0, (3.0, 1.0), 1, q), (0, (3.0, 2.0), 2, r)], expect={"features": 4, "tracks": 2})
    # a path whose links come even ones last to first, then the odd ones: the feature ids jump along the path
    links = list(range(298, -1, -2)) + list(range(1, 299, 2))
    out["path_300"] = _flatten(300, _path(list(range(300)), links), expect={"features": 300, "tracks": 1, "components": 1})
    calls = []
    for k, size in enumerate((63, 64, 65, 130)):   # the lane-class edges: four paths over the same views, scrambled
        calls += _path(list(range(size)), _scrambled(size - 1, 10 + k), k=k + 1)
    out["lane_class_edges"] = _flatten(130, calls, expect={"features": 63 + 64 + 65 + 130, "tracks": 4})
    out["min_length_three"] = _flatten(3, [(0, p, 1, q), (0, r, 1, s), (1, s, 2, r)], min_track_length=3, expect={"small": 1, "tracks": 1})
    a1, b1, c1, a2 = (1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, 4.0)
    out["duplicate_view"] = _flatten(3, [(0, a1, 1, b1), (1, b1, 2, c1), (2, c1, 0, a2)], expect={"inconsistent": 1, "tracks": 1})
    # A match joins two views, so a component of two or more features always keeps two observations: a track falls below two only as a component
    # of ONE feature, which takes min_track_length = 1 and a refused union (here the chain's third feature)
    out["degenerate"] = _flatten(3, [(0, a1, 1, b1), (1, b1, 2, c1)], min_track_length=1, max_track_length=2,
                                 expect={"degenerate": 1, "replayed": 1, "tracks": 1})
    out["max_length_chain"] = _flatten(10, _path(list(range(10)), list(range(9))), max_track_length=4, expect={"replayed": 1})
    out["max_length_chain_scrambled"] = _flatten(10, _path(list(range(10)), _scrambled(9, 3)), max_track_length=4, expect={"replayed": 1})
    tri = lambda v: [(v[0], _pix(v[0], 0), v[1], _pix(v[1], 0)), (v[1], _pix(v[1], 0), v[2], _pix(v[2], 0)), (v[0], _pix(v[0], 0), v[2], _pix(v[2], 0))]
    out["two_triangles_joined_late"] = _flatten(8, tri((0, 1, 2)) + tri((3, 4, 5)) + [(6, p, 7, q), (2, _pix(2, 0), 3, _pix(3, 0))], max_track_length=4,
                                                expect={"replayed": 1, "tracks": 3})
    rng = np.random.RandomState(5)
    calls = []
    for _ in range(240):   # random matches between a few pixels of 12 views: shared features, duplicate views, one large component
        a, b = rng.choice(12, 2, replace=False)
        calls.append((int(a), _pix(int(a), int(rng.randint(6))), int(b), _pix(int(b), int(rng.randint(6)))))
    out["random_mix"] = _flatten(12, calls)
    out["random_mix_max_5"] = _flatten(12, calls, max_track_length=5, min_track_length=3)
    out["probe_chains"] = _flatten(12, calls, hash_capacity_log2=min_capacity_log2(len(calls)))
    out["probe_chains_path"] = _flatten(300, _path(list(range(300)), links), hash_capacity_log2=min_capacity_log2(299))
    out["edge_without_matches"] = _flatten(4, [(0, 1), (0, p, 2, q), (1, 3), (1, 3), (2, q, 3, r), (0, 3)], expect={"tracks": 1, "features": 3})
    out["no_matches"] = _flatten(3, [(0, 1), (1, 2)], expect={"tracks": 0, "features": 0})
    out["no_edges"] = _flatten(3, [], expect={"tracks": 0})
    return out


def non_finite_case():
    return _flatten(3, [(0, (1.0, 2.0), 1, (3.0, 4.0)), (1, (3.0, float("inf")), 2, (5.0, 6.0))])


def call_arguments(case):
    return dict(n_views=case["n_views"], edge_i=case["edge_i"], edge_j=case["edge_j"], match_ptr=case["match_ptr"], matches=case["matches"],
                min_track_length=case["min_track_length"], max_track_length=case["max_track_length"])


# ---- the end-to-end scene: a synthetic track scene written as the COLMAP branch reads it -------------------------------------------------
FLAGS = ("intrinsics_to_optimize: FOCAL_LENGTH\nmin_track_length: 2\nmax_track_length: 1000\nmin_num_inliers_for_valid_match: 5\n"
         "bundle_adjustment_robust_loss_function: HUBER\nbundle_adjustment_robust_loss_width: 10.0\nnum_retriangulation_iterations: 1\n")


def sfm_module():
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "globalsfmpy_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import GlobalSfMpy
    return GlobalSfMpy


def write_colmap_scene(path, n_cams=8, n_tracks=150, seed=4):
    """synth.make_tracks' scene (8 views, about 150 points, half a pixel of noise) as <path>/two_views.txt -- every pair of a track's
    observations is a match of that view pair, the relative pose is the ground truth's -- plus <path>/images/*.png (header-only, the
    size gives the principal point) and <path>/flags.yaml.  Returns the images' wildcard."""
    import os
    from globalsfmpy_amd import dataset_1dsfm as ds, synth
    sc = synth.make_tracks(n_cams, n_tracks, seed, lengths=(2, 3, 4, 5, 8))
    os.makedirs(os.path.join(path, "images"), exist_ok=True)
    names = ["img_%02d.png" % k for k in range(n_cams)]
    for k in range(n_cams):
        ds._fake_png(os.path.join(path, "images", names[k]), int(2 * sc["intrinsics"][k, 1]), int(2 * sc["intrinsics"][k, 2]))
    pairs = {}
    tp = sc["track_ptr"].astype(np.int64)
    for t in range(n_tracks):
        for a in range(tp[t], tp[t + 1]):
            for b in range(a + 1, tp[t + 1]):
                i, j, xa, xb = int(sc["obs_cam"][a]), int(sc["obs_cam"][b]), sc["obs_xy"][a], sc["obs_xy"][b]
                if i > j:
                    i, j, xa, xb = j, i, xb, xa
                pairs.setdefault((i, j), []).append((xa, xb))
    R = synth.aa_to_matrix(sc["rot_aa"])
    with open(os.path.join(path, "two_views.txt"), "w") as f:
        f.write("# img_name1 image_name2 f1 f2 num_inlier rot[0] rot[1] rot[2] trans[0] trans[1] trans[2]\n# features1\n# features2\n")
        for (i, j), m in sorted(pairs.items()):
            rot = synth.quat_to_aa(synth.matrix_to_quat((R[j] @ R[i].T)[None]))[0]
            pos = R[i] @ (sc["cam_pos"][j] - sc["cam_pos"][i])
            pos /= np.linalg.norm(pos)
            f.write("%s %s %.17g %.17g %d %s %s\n" % (names[i], names[j], sc["intrinsics"][i, 0], sc["intrinsics"][j, 0], len(m),
                                                      " ".join("%.17g" % v for v in rot), " ".join("%.17g" % v for v in pos)))
            f.write(" ".join("%.17g %.17g" % (xa[0], xa[1]) for xa, _ in m) + " \n")
            f.write(" ".join("%.17g %.17g" % (xb[0], xb[1]) for _, xb in m) + " \n")
    with open(os.path.join(path, "flags.yaml"), "w") as f:
        f.write(FLAGS)
    return os.path.join(path, "images", "*.png")


def reference_of_reconstruction(rec, min_track_length=2, max_track_length=1000):
    """the restatement on the matches a reconstruction carries (MatchedFeatures(): the arrays CheckView() hands the builder)"""
    em = rec.MatchedFeatures()
    views = sorted({int(v) for v in em["edges"].reshape(-1)})
    dense = {v: k for k, v in enumerate(views)}
    edge_i = np.array([dense[int(v)] for v in em["edges"][:, 0]], dtype=np.uint32)
    edge_j = np.array([dense[int(v)] for v in em["edges"][:, 1]], dtype=np.uint32)
    return build_tracks_reference(len(views), edge_i, edge_j, em["match_ptr"], em["matches"], min_track_length, max_track_length), views
