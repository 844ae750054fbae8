// The tracks of the point-to-camera constraints of position estimation: Theia's NonlinearPositionEstimator::FindTracksForProblem /
// GetTracksSortedByNumViews (reference src/GSfM_nonlinear_position_estimator.cpp:410-506) restated on a track CSR over view ids, and the
// weight of AddPointToCameraConstraints (:389-392).  Plain C++ over std::vector, no HIP and no Theia types: tests/cpp/
// position_track_selection_test.cpp builds it with the host compiler alone.
//
// The reference walks its positions in hash order and breaks ties of its partial_sort as libstdc++ happens to; here both are fixed:
//   views        the views that have a position, in ascending ViewId;
//   skipped      a view with fewer features (observations) than min_num_points_per_view, as the reference skips it (a view the
//                reconstruction does not know has none);
//   candidates   the view's tracks that are not chosen yet, by NumViews (distinct views of the track) descending, then TrackId ascending;
//   taken        in that order until the view's credit reaches the minimum -- a view that earlier tracks credited enough takes none;
//   credit       every view of a chosen track that has a position gets one (the views without a position get none).
// The sum of the credits is the reference's num_point_to_camera_constraints.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

namespace gsfm {

struct PositionTrackSelection {
  std::vector<uint64_t> tracks;                    // the chosen tracks, ascending
  std::unordered_map<uint32_t, int> credits;       // per view with a position
  uint64_t num_point_to_camera_constraints = 0;    // the sum of the credits
};

// track_ptr (n_tracks + 1) / obs_view: the tracks' observations by view id (a view listed twice in a track counts once as a view of the
// track and once per listing as a feature of the view).  positioned_views: any order, no repeats.
inline PositionTrackSelection SelectTracksForPositionEstimation(const std::vector<uint32_t>& positioned_views, uint64_t n_tracks, const uint64_t* track_ptr,
                                                                const uint32_t* obs_view, int min_num_points_per_view) {
  PositionTrackSelection out;
  std::vector<uint32_t> views(positioned_views);
  std::sort(views.begin(), views.end());
  for (uint32_t v : views) out.credits[v] = 0;
  if (min_num_points_per_view <= 0) return out;   // (the zero value: nothing is chosen)
  // per track its distinct views; per positioned view its tracks (distinct, ascending) and its number of features
  std::vector<std::vector<uint32_t>> track_views(n_tracks);
  std::unordered_map<uint32_t, std::vector<uint64_t>> view_tracks;
  std::unordered_map<uint32_t, size_t> num_features;
  for (uint64_t t = 0; t < n_tracks; ++t) {
    std::vector<uint32_t>& tv = track_views[t];
    tv.assign(obs_view + track_ptr[t], obs_view + track_ptr[t + 1]);
    for (uint32_t v : tv) if (out.credits.count(v)) ++num_features[v];
    std::sort(tv.begin(), tv.end());
    tv.erase(std::unique(tv.begin(), tv.end()), tv.end());
    for (uint32_t v : tv) if (out.credits.count(v)) view_tracks[v].push_back(t);
  }
  std::vector<uint8_t> chosen(n_tracks, 0);
  for (uint32_t v : views) {
    if (num_features[v] < (size_t)min_num_points_per_view) continue;
    std::vector<std::pair<uint64_t, size_t>> cand;   // (track, NumViews) of the tracks not chosen when the view's turn comes
    for (uint64_t t : view_tracks[v]) if (!chosen[t]) cand.emplace_back(t, track_views[t].size());
    std::sort(cand.begin(), cand.end(), [](const std::pair<uint64_t, size_t>& a, const std::pair<uint64_t, size_t>& b) {
      return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    for (size_t i = 0; i < cand.size() && out.credits[v] < min_num_points_per_view; ++i) {
      chosen[cand[i].first] = 1;
      for (uint32_t w : track_views[cand[i].first]) {
        auto it = out.credits.find(w);
        if (it != out.credits.end()) ++it->second;
      }
    }
  }
  for (uint64_t t = 0; t < n_tracks; ++t) if (chosen[t]) out.tracks.push_back(t);
  for (const auto& kv : out.credits) out.num_point_to_camera_constraints += (uint64_t)kv.second;
  return out;
}

// AddPointToCameraConstraints' weight: the option times (camera-to-camera residuals) / (point-to-camera constraints)
inline double PointToCameraWeight(double point_to_camera_weight, uint64_t num_camera_to_camera, uint64_t num_point_to_camera) {
  return point_to_camera_weight * (double)num_camera_to_camera / (double)num_point_to_camera;
}

}  // namespace gsfm
