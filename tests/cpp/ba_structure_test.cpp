// The host structure of a bundle-adjustment problem (csrc/ba_structure.hpp), built by the host compiler alone: no HIP header, no device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "ba_structure.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

using U32 = std::vector<uint32_t>;
using U8 = std::vector<uint8_t>;

int main() {
  {
    // 4 cameras (camera 2 unestimated, camera 3 in no observation), 4 tracks (track 1 unestimated, track 3 seen by camera 2 alone):
    //   track 0: obs 0 (cam 0), 1 (cam 1), 2 (cam 2)   track 1: obs 3 (cam 0), 4 (cam 1)   track 2: obs 5 (cam 1), 6 (cam 0), 7 (cam 1)   track 3: obs 8 (cam 2)
    const std::vector<uint64_t> ptr = {0, 3, 5, 8, 9};
    const U32 cam = {0, 1, 2, 0, 1, 1, 0, 1, 2};
    const U8 cam_est = {1, 1, 0, 1}, pt_est = {1, 0, 1, 1};
    const BaStructure s = ba_build_structure(4, cam_est.data(), 4, ptr.data(), cam.data(), pt_est.data());
    CHECK((s.row_ptr == U32{0, 2, 5, 5, 5}));
    CHECK((s.obs == U32{0, 6, 1, 5, 7}));
    CHECK((s.trk == U32{0, 2, 0, 2, 2}));
    CHECK((s.cam_active == U8{1, 1, 0, 0}));
    CHECK((s.point_active == U8{1, 0, 1, 0}));
    CHECK((s.track_used == U8{1, 0, 1, 1}));
    CHECK(s.n_used == 5 && s.n_active_cams == 2 && s.n_active_points == 2);
    // NULL flags: everything estimated
    const BaStructure a = ba_build_structure(4, nullptr, 4, ptr.data(), cam.data(), nullptr);
    CHECK(a.n_used == 9 && a.n_active_cams == 3 && a.n_active_points == 4);
    CHECK((a.row_ptr == U32{0, 3, 7, 9, 9}));
    CHECK((a.obs == U32{0, 3, 6, 1, 4, 5, 7, 2, 8}));
  }
  {
    // nothing at all, and tracks without observations
    const std::vector<uint64_t> ptr0 = {0};
    const BaStructure e = ba_build_structure(0, nullptr, 0, ptr0.data(), nullptr, nullptr);
    CHECK(e.row_ptr == U32{0} && e.n_used == 0 && e.obs.empty());
    const std::vector<uint64_t> ptr2 = {0, 0, 0};
    const BaStructure f = ba_build_structure(2, nullptr, 2, ptr2.data(), nullptr, nullptr);
    CHECK((f.row_ptr == U32{0, 0, 0}) && f.n_active_cams == 0 && f.n_active_points == 0);
  }
  {
    // 150 cameras, 2000 random tracks of 0 .. 12 observations with repeated cameras and random flags, against a plain stable sort
    const uint32_t N = 150, T = 2000;
    std::mt19937 rng(11);
    std::vector<uint64_t> ptr(T + 1, 0);
    U32 cam;
    U8 cam_est(N), pt_est(T);
    for (uint32_t k = 0; k < N; ++k) cam_est[k] = rng() % 10 != 0;
    for (uint32_t t = 0; t < T; ++t) {
      pt_est[t] = rng() % 8 != 0;
      const uint32_t len = rng() % 13;
      for (uint32_t k = 0; k < len; ++k) cam.push_back(rng() % N);
      ptr[t + 1] = cam.size();
    }
    const BaStructure s = ba_build_structure(N, cam_est.data(), T, ptr.data(), cam.data(), pt_est.data());
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> want;   // camera, observation, track
    for (uint32_t t = 0; t < T; ++t)
      for (uint64_t e = ptr[t]; e < ptr[t + 1]; ++e)
        if (pt_est[t] && cam_est[cam[e]]) want.emplace_back(cam[e], (uint32_t)e, t);
    std::sort(want.begin(), want.end());
    CHECK(s.n_used == want.size() && s.obs.size() == want.size() && s.trk.size() == want.size() && s.row_ptr.size() == N + 1);
    std::vector<uint32_t> deg(N, 0);
    U8 pa(T, 0);
    for (size_t d = 0; d < want.size() && d < s.obs.size(); ++d) {
      const auto [k, e, t] = want[d];
      deg[k]++; pa[t] = 1;
      CHECK(s.row_ptr[k] <= d && d < s.row_ptr[k + 1]);
      CHECK(s.obs[d] == e && s.trk[d] == t);
    }
    for (uint32_t k = 0; k < N; ++k) { CHECK(s.row_ptr[k + 1] - s.row_ptr[k] == deg[k]); CHECK(s.cam_active[k] == (deg[k] > 0)); }
    CHECK(s.point_active == pa);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("PASSED\n");
  return 0;
}
