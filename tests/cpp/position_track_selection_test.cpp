// The tracks of the point-to-camera constraints (include/gsfm/position_track_selection.hpp), built by the host compiler alone: no HIP header,
// no device.  tests/test_position_track_selection.py also builds it with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gsfm/position_track_selection.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

using U32 = std::vector<uint32_t>;
using U64 = std::vector<uint64_t>;

int main() {
  {
    // views 1 .. 5 have positions, view 9 has none.  tracks:
    //   0: 1 2        1: 1 2 3      2: 1 3 9 (three views, one without a position)    3: 2 3 4     4: 4 5     5: 5 9     6: 3 4 5
    const U64 ptr = {0, 2, 5, 8, 11, 13, 15, 18};
    const U32 view = {1, 2, 1, 2, 3, 1, 3, 9, 2, 3, 4, 4, 5, 5, 9, 3, 4, 5};
    const U32 positioned = {5, 3, 1, 2, 4};   // (any order)
    const gsfm::PositionTrackSelection s = gsfm::SelectTracksForPositionEstimation(positioned, 7, ptr.data(), view.data(), 2);
    // view 1 (3 features): candidates 1, 2 (three views each: the tie goes to the smaller id), then 0 -> takes 1 and 2: credits 1:2 2:1 3:2
    // view 2 (3 features, credit 1): candidates 3 (three views), 0 -> takes 3: credits 2:2 3:3 4:1
    // view 3 (credit 3): credited by earlier tracks, takes none
    // view 4 (3 features, credit 1): candidates 6 (three views), 4 -> takes 6: credits 3:4 4:2 5:1
    // view 5 (3 features, credit 1): candidates 4, 5 (two views each) -> takes 4: credits 4:3 5:2
    CHECK((s.tracks == U64{1, 2, 3, 4, 6}));
    CHECK(s.credits.at(1) == 2 && s.credits.at(2) == 2 && s.credits.at(3) == 4 && s.credits.at(4) == 3 && s.credits.at(5) == 2);
    CHECK(s.credits.count(9) == 0 && s.num_point_to_camera_constraints == 13);
    CHECK(gsfm::PointToCameraWeight(0.5, 26, 13) == 1.0);
    // a minimum above a view's features: the view is skipped, but still credited by the tracks of other views
    const gsfm::PositionTrackSelection big = gsfm::SelectTracksForPositionEstimation(positioned, 7, ptr.data(), view.data(), 4);
    // only view 3 has four features (tracks 1, 2, 3, 6): it takes all four
    CHECK((big.tracks == U64{1, 2, 3, 6}));
    CHECK(big.credits.at(3) == 4 && big.credits.at(1) == 2 && big.credits.at(2) == 2 && big.credits.at(4) == 2 && big.credits.at(5) == 1);
    // the zero value chooses nothing; no positions, no credits
    CHECK(gsfm::SelectTracksForPositionEstimation(positioned, 7, ptr.data(), view.data(), 0).tracks.empty());
    const gsfm::PositionTrackSelection none = gsfm::SelectTracksForPositionEstimation({}, 7, ptr.data(), view.data(), 2);
    CHECK(none.tracks.empty() && none.num_point_to_camera_constraints == 0);
    const gsfm::PositionTrackSelection empty = gsfm::SelectTracksForPositionEstimation(positioned, 0, U64{0}.data(), nullptr, 2);
    CHECK(empty.tracks.empty() && empty.credits.size() == 5);
  }
  {
    // random tracks: every positioned view with enough features ends with at least the minimum, and the credits are what the chosen tracks give
    std::mt19937 rng(3);
    const uint32_t V = 40;
    U64 ptr = {0};
    U32 view;
    for (int t = 0; t < 300; ++t) {
      const int len = 2 + rng() % 5;
      for (int k = 0; k < len; ++k) view.push_back(rng() % V);   // (a view may repeat within a track: one view, several features)
      ptr.push_back(view.size());
    }
    U32 positioned;
    for (uint32_t v = 0; v < V; v += 1 + v % 2) positioned.push_back(v);
    for (int min_points : {1, 3, 8}) {
      const gsfm::PositionTrackSelection s = gsfm::SelectTracksForPositionEstimation(positioned, 300, ptr.data(), view.data(), min_points);
      std::vector<int> credit(V, 0), features(V, 0), distinct_tracks(V, 0);
      for (uint64_t t = 0; t < 300; ++t) {
        std::vector<uint8_t> seen(V, 0);
        for (uint64_t e = ptr[t]; e < ptr[t + 1]; ++e) { ++features[view[e]]; if (!seen[view[e]]) { seen[view[e]] = 1; ++distinct_tracks[view[e]]; } }
      }
      for (uint64_t t : s.tracks) {
        std::vector<uint8_t> seen(V, 0);
        for (uint64_t e = ptr[t]; e < ptr[t + 1]; ++e) if (!seen[view[e]]) { seen[view[e]] = 1; ++credit[view[e]]; }
      }
      uint64_t sum = 0;
      for (uint32_t v : positioned) {
        CHECK(s.credits.at(v) == credit[v]);
        if (features[v] >= min_points) CHECK(credit[v] >= std::min(min_points, distinct_tracks[v]));
        sum += credit[v];
      }
      CHECK(sum == s.num_point_to_camera_constraints && s.credits.size() == positioned.size());
    }
  }
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
