// The plain part of csrc/track_scene.hpp, built by the host compiler alone: the lane classes at their boundaries, the launch order, the
// estimated-only launch order of the outlier rule, and every refusal of the track-array checks under each size rule and both settings of
// the track_ptr[0] check, with which fault of two is reported.  Prints PASSED.
#include <cstdio>
#include <string>
#include <vector>

#include "track_scene.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

typedef std::vector<uint64_t> U64;
typedef std::vector<uint32_t> U32;
static const uint64_t BIG = 1ull << 31;
static const TrackLimit LIMITS[3] = {TrackLimit::tracks, TrackLimit::tracks_and_lengths, TrackLimit::observations_and_nodes};

static U64 ptr_of(const U64& lengths) {
  U64 p(1, 0);
  for (uint64_t n : lengths) p.push_back(p.back() + n);
  return p;
}

// "" when track_ptr_ok accepts, else its message
static std::string ptr_says(uint64_t n_tracks, const uint64_t* track_ptr, TrackLimit limit, uint64_t cam_nodes, bool first_is_zero, const char* null_message = "NULL") {
  std::string why = "untouched";
  const bool ok = track_ptr_ok(n_tracks, track_ptr, limit, cam_nodes, first_is_zero, null_message, &why);
  CHECK(ok == (why == "untouched"));
  return ok ? "" : why;
}
static std::string obs_says(uint32_t n_cams, const U32& cam, bool have_xy) {
  std::string why = "untouched";
  const double xy[16] = {};
  const bool ok = track_obs_ok(n_cams, cam.size(), cam.empty() ? nullptr : cam.data(), have_xy ? xy : nullptr, &why);
  CHECK(ok == (why == "untouched"));
  return ok ? "" : why;
}

static void test_classes_and_order() {
  const uint64_t G4 = TRI_LEN_G4, G16 = TRI_LEN_G16;
  CHECK(tri_class_of(0) == 0 && tri_class_of(G4) == 0 && tri_class_of(G4 + 1) == 1 && tri_class_of(G16) == 1 && tri_class_of(G16 + 1) == 2);
  CHECK(tri_class_of(BIG) == 2);
  // tracks:                   0   1       2   3    4        5  6   7       8        9
  const U64 p = ptr_of({2, G4, G16 + 1, 0, G16, G4 + 1, 2, G4, G16 + 9, G16});
  U32 order(10, 99);
  uint64_t cb[4] = {9, 9, 9, 9};
  tri_bucket(10, p.data(), order.data(), cb);
  CHECK(cb[0] == 0 && cb[1] == 5 && cb[2] == 8 && cb[3] == 10);
  CHECK((order == U32{1, 7, 0, 6, 3, 4, 9, 5, 8, 2}));   // descending length inside a class, equal lengths by track index
  uint64_t none[4] = {9, 9, 9, 9};
  tri_bucket(0, p.data(), nullptr, none);
  CHECK(none[0] == 0 && none[1] == 0 && none[2] == 0 && none[3] == 0);
}

static void test_keep_estimated() {
  const uint64_t G4 = TRI_LEN_G4, G16 = TRI_LEN_G16;
  const U64 p = ptr_of({2, G4, G16 + 1, 0, G16, G4 + 1, 2, G4, G16 + 9, G16});
  U32 full(10);
  uint64_t all[4];
  tri_bucket(10, p.data(), full.data(), all);
  struct Case { std::vector<uint8_t> flags; U32 order; uint64_t cb[4]; };
  const Case cases[] = {
      {{1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, {1, 7, 0, 6, 3, 4, 9, 5, 8, 2}, {0, 5, 8, 10}},
      {{0, 0, 1, 0, 1, 1, 0, 0, 1, 0}, {4, 5, 8, 2}, {0, 0, 2, 4}},            // the first class empty
      {{1, 0, 1, 1, 0, 0, 1, 1, 0, 0}, {7, 0, 6, 3, 2}, {0, 4, 4, 5}},         // the middle class empty
      {{0, 1, 0, 1, 0, 1, 0, 0, 0, 1}, {1, 3, 9, 5}, {0, 2, 4, 4}},            // the last class empty
      {{0, 0, 0, 0, 7, 0, 0, 0, 0, 0}, {4}, {0, 0, 1, 1}},                     // (any non-zero byte is a flag)
      {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {}, {0, 0, 0, 0}}};                     // no track estimated
  for (const Case& c : cases) {
    U32 order = full;
    uint64_t cb[4] = {9, 9, 9, 9};
    const uint64_t n = tri_keep_estimated(order.data(), all, c.flags.data(), cb);
    order.resize(n);
    CHECK(n == c.order.size() && order == c.order);
    CHECK(cb[0] == c.cb[0] && cb[1] == c.cb[1] && cb[2] == c.cb[2] && cb[3] == c.cb[3]);
  }
  U32 order = full;
  uint64_t cb[4];
  CHECK(tri_keep_estimated(order.data(), all, nullptr, cb) == 10 && order == full && cb[1] == 5 && cb[2] == 8 && cb[3] == 10);   // no flags: all
}

static void test_track_ptr_checks() {
  const U64 good = {0, 2, 4}, first1 = {1, 2, 4}, down = {0, 3, 2, 4}, first1_down = {1, 3, 2, 4}, long0 = {0, BIG, BIG + 1}, long0_down = {0, BIG, 2};
  const U64 many_obs = {0, BIG - 1, BIG}, one_short = {0, BIG - 2, BIG - 1};
  for (TrackLimit limit : LIMITS)
    for (int zero = 0; zero < 2; ++zero) {
      const bool lengths = limit == TrackLimit::tracks_and_lengths, nodes = limit == TrackLimit::observations_and_nodes;
      CHECK(ptr_says(2, good.data(), limit, 3, zero) == "");
      CHECK(ptr_says(0, good.data(), limit, 3, zero) == "");
      // NULL: the caller's words, before everything else; no words: the caller has looked, and nothing is read of no tracks (but the
      // bundle adjustments' count of observations, track_ptr[0])
      CHECK(ptr_says(2, nullptr, limit, 3, zero, "the caller's words") == "the caller's words");
      CHECK(ptr_says(BIG, nullptr, limit, BIG, zero) == "NULL");
      if (!zero && !nodes) CHECK(ptr_says(0, nullptr, limit, 3, false, nullptr) == "");
      // 2^31 tracks: refused before track_ptr is read (one entry here) -- by the bundle adjustments only after the walk, as nodes
      if (!nodes) CHECK(ptr_says(BIG, first1.data(), limit, 0, zero) == "problem too large (2^31 tracks)");
      if (!nodes) CHECK(ptr_says(BIG - 1, first1.data(), limit, 0, true) == "track_ptr[0] must be 0");
      // track_ptr[0]
      CHECK(ptr_says(2, first1.data(), limit, 3, zero) == (zero ? "track_ptr[0] must be 0" : ""));
      CHECK(ptr_says(3, first1_down.data(), limit, 3, zero) == (zero ? "track_ptr[0] must be 0" : "track_ptr decreases at track 1"));
      // the walk: the first track with a fault, and of its two faults the decrease
      CHECK(ptr_says(3, down.data(), limit, 3, zero) == "track_ptr decreases at track 1");
      CHECK(ptr_says(2, long0.data(), limit, 3, zero) == (lengths ? "track 0 is too long (2^31 observations)" : nodes ? "problem too large (2^31 observations or nodes)" : ""));
      CHECK(ptr_says(2, long0_down.data(), limit, 3, zero) == (lengths ? "track 0 is too long (2^31 observations)" : "track_ptr decreases at track 1"));
      CHECK(ptr_says(1, long0.data() + 1, limit, 3, false) == (nodes ? "problem too large (2^31 observations or nodes)" : ""));   // a track of 1 from 2^31 on
      // the bundle adjustments' size: observations, or cam_nodes + n_tracks nodes
      CHECK(ptr_says(2, many_obs.data(), limit, 3, zero) == (nodes ? "problem too large (2^31 observations or nodes)" : ""));
      CHECK(ptr_says(2, one_short.data(), limit, 3, zero) == "");
      CHECK(ptr_says(2, good.data(), limit, BIG - 2, zero) == (nodes ? "problem too large (2^31 observations or nodes)" : ""));
      CHECK(ptr_says(2, good.data(), limit, BIG - 3, zero) == "");
    }
}

static void test_observation_checks() {
  CHECK(obs_says(3, {0, 1, 2, 0}, true) == "");
  CHECK(obs_says(0, {}, false) == "");   // no observations: neither array is looked at
  CHECK(obs_says(3, {0, 1, 3, 0}, true) == "observation 2 has an out-of-range camera index");
  CHECK(obs_says(3, {7, 1, 3, 0}, true) == "observation 0 has an out-of-range camera index");
  CHECK(obs_says(0, {0}, true) == "observation 0 has an out-of-range camera index");
  CHECK(obs_says(3, {0, 1, 3, 0}, false) == "NULL argument");   // before the indices
  std::string why;
  const double xy[2] = {};
  CHECK(!track_obs_ok(3, 1, nullptr, xy, &why) && why == "NULL argument");
}

int main() {
  test_classes_and_order();
  test_keep_estimated();
  test_track_ptr_checks();
  test_observation_checks();
  std::printf(failures ? "%d checks FAILED\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
