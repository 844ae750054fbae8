// Device kernel of the outlier rule (include/gsfm_tracks.h, gsfm_tracks_outlier_tracks): Theia's SetOutlierTracksToUnestimated under the
// definition of that header.
//
//   k_outlier_tracks<G>  the lane group, the lane classes and the launch order of k_tri_tracks<G> (triangulate_kernels.hpp), over the tracks
//                        that are estimated on input only (the host filters gsfm_tracks_launch_order's order; the others are not launched).
//                rays    lane l of the group takes observations l, l + G, ... of the track: the unit ray d = (X - o) / |X - o| from the
//                        camera centre to the track's POINT goes to the ray store of tri_track (NaN for an observation of an unestimated
//                        camera, and for a point at a camera centre: neither passes a comparison);
//                gate    tri_gate<G>, the text of the triangulation: the behind flag and the mean squared pixel error, to the bit;
//                angle   tri_angle<G>, the sweep of the triangulation over the ray store.
// The ray store is written and read by different lanes of ONE wavefront: a work-group fence orders the two.  No atomics, nothing waits for
// another work-group, every loop is bounded by the track's CSR length.  The lanes of a group are active together or not at all, so every
// shuffle and ballot of a group is executed by all of its lanes (the rule of k_tri_tracks); the early exits are taken by whole groups.
#pragma once
#include "triangulate_kernels.hpp"

namespace gsfm {

struct OutlierArgs {
  TriArgs tri;            // order: the estimated tracks of the class; point is not used; status, n_views and mean_sq_err are the outputs
  const double* points;   // [3 x n_tracks], the input
};

template <int G>
__global__ void __launch_bounds__(G == 64 ? 64 : GSFM_TRI_BLOCK) k_outlier_tracks(OutlierArgs oa) {
  constexpr int BLOCK = G == 64 ? 64 : GSFM_TRI_BLOCK;
  constexpr int GROUPS = BLOCK / G;
  constexpr int CAP = G == 4 ? GSFM_TRI_LEN_G4 : GSFM_TRI_LEN_G16;
  __shared__ double lds_rays[G == 64 ? 1 : 3 * GROUPS * CAP];
  const TriArgs& a = oa.tri;
  const int group = threadIdx.x / G, l = threadIdx.x % G, lane_in_wave = threadIdx.x & 63;
  const TriTrack tk = tri_track<G>(a, lds_rays, group);
  double X[3] = {0.0, 0.0, 0.0};
  if (tk.live) { X[0] = oa.points[3 * tk.t]; X[1] = oa.points[3 * tk.t + 1]; X[2] = oa.points[3 * tk.t + 2]; }
  // ---- the rays from the camera centres to the point ----
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int mine = 0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const double* cam = a.cams + (uint64_t)GSFM_TRI_CAM_DOUBLES * a.obs_cam[tk.ob + k];
    double d0 = nan, d1 = nan, d2 = nan;
    if (cam[15] != 0.0) {
      const double v0 = X[0] - cam[9], v1 = X[1] - cam[10], v2 = X[2] - cam[11];
      const double nrm = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
      d0 = v0 / nrm; d1 = v1 / nrm; d2 = v2 / nrm;
      ++mine;
    }
    tk.rx[k] = d0; tk.ry[k] = d1; tk.rz[k] = d2;
  }
  __threadfence_block();   // the rays are read by the group's other lanes in tri_angle
  const int n = tri_group_allsum_int<G>(mine);
  double mean;
  int status;
  if (tri_gate<G>(a, tk, l, lane_in_wave, X, n, mean) == 4) status = 2;
  else if (mean > a.max_sq_err) status = 3;   // strict, and false for a NaN mean
  else status = tri_angle<G>(tk, l, lane_in_wave, a.cos_min_angle) ? 0 : 4;
  if (tk.live && l == 0) {
    a.status[tk.t] = status;
    a.n_views[tk.t] = n;
    a.mean_sq_err[tk.t] = mean;
  }
}

}  // namespace gsfm
