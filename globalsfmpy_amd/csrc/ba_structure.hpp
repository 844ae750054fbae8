// The host structure of a bundle-adjustment problem (solver_ba.hpp): which observations are used, which cameras and points are active,
// and the per-camera CSR of the used observations.  Host vectors in, host vectors out, no HIP: tests/cpp/ba_structure_test.cpp builds it
// with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// An observation (place e of the track CSR) is USED when its camera and its track are both estimated.  A camera or a point with no used
// observation is inactive.  Row k of the camera CSR lists camera k's used observations in ascending e (a stable counting sort of the
// track-ordered observations by camera): obs[d] is the observation of entry d, trk[d] its track.
struct BaStructure {
  std::vector<uint32_t> row_ptr, obs, trk;   // n_cams + 1, n_used, n_used
  std::vector<uint8_t> cam_active, point_active, track_used;   // track_used: the track is estimated (its observations in estimated cameras are used)
  uint64_t n_used = 0;
  uint32_t n_active_cams = 0;
  uint64_t n_active_points = 0;
};

// (the camera indices are in range, track_ptr ascends from 0 and the observations fit 32 bits: the caller has checked)
BaStructure ba_build_structure(uint32_t n_cams, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                               const uint8_t* point_estimated) {
  const size_t N = n_cams, T = n_tracks;
  BaStructure s;
  s.row_ptr.assign(N + 1, 0);
  s.cam_active.assign(N, 0); s.point_active.assign(T, 0); s.track_used.assign(T, 0);
  auto cam_ok = [&](uint32_t k) { return !cam_estimated || cam_estimated[k] != 0; };
  for (size_t t = 0; t < T; ++t) {
    if (point_estimated && !point_estimated[t]) continue;
    s.track_used[t] = 1;
    for (uint64_t e = track_ptr[t]; e < track_ptr[t + 1]; ++e)
      if (cam_ok(obs_cam[e])) { s.row_ptr[obs_cam[e] + 1]++; s.point_active[t] = 1; }
  }
  for (size_t k = 0; k < N; ++k) { s.cam_active[k] = s.row_ptr[k + 1] > 0; s.row_ptr[k + 1] += s.row_ptr[k]; }
  s.n_used = s.row_ptr[N];
  s.obs.resize(s.n_used); s.trk.resize(s.n_used);
  std::vector<uint32_t> fill(s.row_ptr.begin(), s.row_ptr.end() - 1);
  for (size_t t = 0; t < T; ++t) {
    if (!s.track_used[t]) continue;
    for (uint64_t e = track_ptr[t]; e < track_ptr[t + 1]; ++e)
      if (cam_ok(obs_cam[e])) { const uint32_t d = fill[obs_cam[e]]++; s.obs[d] = (uint32_t)e; s.trk[d] = (uint32_t)t; }
  }
  for (size_t k = 0; k < N; ++k) s.n_active_cams += s.cam_active[k];
  for (size_t t = 0; t < T; ++t) s.n_active_points += s.point_active[t];
  return s;
}

}  // namespace
