// Device kernels of the track triangulation (include/gsfm_tracks.h, gsfm_tracks_triangulate): Theia's TrackEstimator::EstimateTrack
// without the per-track refinement, under the definition of that header.
//
// A LANE GROUP of G lanes owns one track; G is 4, 16 or 64 by the track's length alone (GSFM_TRI_LEN_G4 / GSFM_TRI_LEN_G16), one launch
// per class.  Real tracks are mostly shorter than 8 observations: a wavefront per track would idle almost every lane, a lane per track
// would serialise the O(n^2) angle test of the long ones.  A group never spans two wavefronts, so nothing here needs a barrier.
//
//   k_tri_cameras   one lane per camera: R(aa), position, f u v and the estimated flag into one 128-byte record, so that an observation
//                   gathers a single cache line and no observation pays for a sincos.
//   k_tri_tracks<G> pass 1  lane l of the group takes observations l, l + G, ... of the track: the unit ray d, computed ONCE, goes to
//                           the ray store (dx | dy | dz planes: LDS for G = 4 and 16, a global plane for G = 64; NaN for an observation
//                           of an unestimated camera, which can then pass no comparison), and the lane's terms of M and q are added
//                           in that order; an xor butterfly over the group gives every lane the same nine sums;
//                   angle   row block i0 = 0, G, ...: lane l holds ray i0 + l in registers, all lanes of the group read ray j together
//                           (one broadcast address) for j = i0 + 1 ..; the group leaves at the first j at which any lane's pair
//                           passes (ballot, masked to the group);
//                   solve   the 3 x 3 Cholesky in every lane;
//                   gate    lane l re-reads its observations' pixels and camera records: depth sign and squared pixel error, butterfly.
// The ray store is written and read by different lanes of ONE wavefront: a work-group fence orders the two.  No atomics, nothing waits
// for another work-group, no host round trip.  Front (pass 1, angle, solve) and gate are __device__ functions: k_tri_refine_tracks
// (track_refine_kernels.hpp) runs the same text around its refinement, and k_outlier_tracks (outlier_kernels.hpp) runs the angle sweep
// (tri_angle) and the gate on a point it is given.  A track's arithmetic depends on its own length and data alone (the class, the lane
// stride and the butterfly are functions of the length), so two calls return the same bytes and so does a call with the tracks permuted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cov_kernels.hpp"

namespace gsfm {

#define GSFM_TRI_LEN_G4 8      // tracks of up to 8 observations: groups of 4 lanes
#define GSFM_TRI_LEN_G16 64    // 9 .. 64 observations: groups of 16 lanes; 65 and more: one wavefront
#define GSFM_TRI_CAM_DOUBLES 16
#define GSFM_TRI_BLOCK 256     // threads per block of the classes 4 and 16 (the class 64 launches one wavefront per block)

struct TriArgs {
  uint64_t n_slots;            // tracks of this class
  const uint32_t* order;       // slot -> track (this class's slice: longest first), outputs stay in caller order
  const uint64_t* track_ptr;   // [n_tracks + 1]
  const uint32_t* obs_cam;
  const double2* obs_xy;       // pixels
  const double* cams;          // GSFM_TRI_CAM_DOUBLES per camera: R row-major (9), position (3), f u v, estimated (1 / 0)
  double* plane;               // class 64 only: 3 x n_obs, dx | dy | dz at the observation's own index
  uint64_t n_obs;
  double cos_min_angle;
  double max_sq_err;
  double* point;
  int32_t* status;
  int32_t* n_views;
  double* mean_sq_err;
};

__global__ void __launch_bounds__(256) k_tri_cameras(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                                     const uint8_t* cam_estimated, double* cams) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  const double w[3] = {rot_aa[3 * (uint64_t)c], rot_aa[3 * (uint64_t)c + 1], rot_aa[3 * (uint64_t)c + 2]};
  double R[9];
  rodrigues(w, R);
  double* o = cams + (uint64_t)GSFM_TRI_CAM_DOUBLES * c;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[9 + k] = cam_pos[3 * (uint64_t)c + k]; o[12 + k] = intrinsics[3 * (uint64_t)c + k]; }
  o[15] = (!cam_estimated || cam_estimated[c]) ? 1.0 : 0.0;
}

template <int G>
__device__ __forceinline__ double tri_group_allsum(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}
template <int G>
__device__ __forceinline__ int tri_group_allsum_int(int v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}
// true in every lane of the group when `flag` holds in any of its lanes; the group's lanes are all active or all inactive together
template <int G>
__device__ __forceinline__ bool tri_group_any(bool flag, int lane_in_wave) {
  const unsigned long long b = __ballot(flag);
  if (G == 64) return b != 0ull;
  return ((b >> (lane_in_wave & ~(G - 1))) & ((1ull << (G & 63)) - 1ull)) != 0ull;
}

// The track of a lane's group and the group's ray store (index k of the store is the observation's place in the track).  A dead group (the
// last block's spare slots) runs along on an empty track and stores nothing.
struct TriTrack {
  bool live;
  uint64_t t, ob;
  uint32_t len;
  double* rx, * ry, * rz;
};
template <int G>
__device__ __forceinline__ TriTrack tri_track(const TriArgs& a, double* lds_rays, int group) {
  constexpr int GROUPS = (G == 64 ? 64 : GSFM_TRI_BLOCK) / G;
  constexpr int CAP = G == 4 ? GSFM_TRI_LEN_G4 : GSFM_TRI_LEN_G16;          // the longest track of the class (LDS classes)
  TriTrack k;
  const uint64_t slot = (uint64_t)blockIdx.x * GROUPS + group;
  k.live = slot < a.n_slots;
  k.t = k.live ? a.order[slot] : 0;
  k.ob = k.live ? a.track_ptr[k.t] : 0;
  const uint64_t oe = k.live ? a.track_ptr[k.t + 1] : 0;
  k.len = (uint32_t)(oe - k.ob);
  if (G == 64) { k.rx = a.plane + k.ob; k.ry = k.rx + a.n_obs; k.rz = k.ry + a.n_obs; }
  else { k.rx = lds_rays + 3 * CAP * group; k.ry = k.rx + CAP; k.rz = k.ry + CAP; }
  return k;
}

// Step 3 of include/gsfm_tracks.h over the group's ray store: true when some pair i < j has d_i . d_j < cos(min angle).  Row block i0 = 0,
// G, ...: lane l holds ray i0 + l in registers and all lanes read ray j together; the group leaves at the first j at which any lane's pair
// passes.  The same value in every lane.  Also the angle test of k_outlier_tracks (outlier_kernels.hpp), whose rays come from the point.
template <int G>
__device__ __forceinline__ bool tri_angle(const TriTrack& tk, int l, int lane_in_wave, double cos_min_angle) {
  const uint32_t len = tk.len;
  const double* const rx = tk.rx, * const ry = tk.ry, * const rz = tk.rz;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  bool found = false;
  for (uint32_t i0 = 0; i0 < len && !found; i0 += G) {
    const uint32_t i = i0 + l;
    double e0 = nan, e1 = nan, e2 = nan;
    if (i < len) { e0 = rx[i]; e1 = ry[i]; e2 = rz[i]; }
    for (uint32_t j = i0 + 1; j < len; ++j) {
      const double dot = e0 * rx[j] + e1 * ry[j] + e2 * rz[j];
      if (tri_group_any<G>(j > i && dot < cos_min_angle, lane_in_wave)) { found = true; break; }
    }
  }
  return found;
}

// Steps 1 to 4 of include/gsfm_tracks.h, the text both track kernels run: the rays and the sums, the angle test, the midpoint.  Returns the
// status (0: X holds the midpoint; 1, 2, 3: X is zero); n is the count of observations in estimated views.  The same values in every lane.
template <int G>
__device__ __forceinline__ int tri_front(const TriArgs& a, const TriTrack& tk, int l, int lane_in_wave, double* X, int& n) {
  const uint64_t ob = tk.ob;
  const uint32_t len = tk.len;
  double* const rx = tk.rx, * const ry = tk.ry, * const rz = tk.rz;
  // ---- pass 1: rays, once, and the sums of M = sum (I - d d^T), q = sum (I - d d^T) o ----
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // M: xx xy xz yy yz zz, q: x y z
  int mine = 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (uint32_t k = l; k < len; k += G) {
    const double* cam = a.cams + (uint64_t)GSFM_TRI_CAM_DOUBLES * a.obs_cam[ob + k];
    double d0 = nan, d1 = nan, d2 = nan;
    if (cam[15] != 0.0) {
      const double2 xy = a.obs_xy[ob + k];
      const double f = cam[12], fx = (xy.x - cam[13]) / f, fy = (xy.y - cam[14]) / f;
      const double r0 = cam[0] * fx + cam[3] * fy + cam[6], r1 = cam[1] * fx + cam[4] * fy + cam[7], r2 = cam[2] * fx + cam[5] * fy + cam[8];
      const double nrm = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
      d0 = r0 / nrm; d1 = r1 / nrm; d2 = r2 / nrm;
      const double o0 = cam[9], o1 = cam[10], o2 = cam[11];
      const double dox = d0 * o0 + d1 * o1 + d2 * o2;
      s[0] += 1.0 - d0 * d0; s[1] -= d0 * d1; s[2] -= d0 * d2; s[3] += 1.0 - d1 * d1; s[4] -= d1 * d2; s[5] += 1.0 - d2 * d2;
      s[6] += o0 - d0 * dox; s[7] += o1 - d1 * dox; s[8] += o2 - d2 * dox;
      ++mine;
    }
    rx[k] = d0; ry[k] = d1; rz[k] = d2;
  }
  __threadfence_block();   // the rays are read by the group's other lanes below
  n = tri_group_allsum_int<G>(mine);
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = tri_group_allsum<G>(s[k]);

  int status = 0;
  X[0] = 0.0; X[1] = 0.0; X[2] = 0.0;
  if (n < 2) status = 1;
  else if (!tri_angle<G>(tk, l, lane_in_wave, a.cos_min_angle)) status = 2;   // the angle: some pair i < j with d_i . d_j < cos(min angle)
  if (status == 0) {
    // ---- M X = q by Cholesky, M = L L^T ----
    const double p0 = s[0];
    const double l00 = sqrt(p0), l10 = s[1] / l00, l20 = s[2] / l00;
    const double p1 = s[3] - l10 * l10;
    const double l11 = sqrt(p1), l21 = (s[4] - l20 * l10) / l11;
    const double p2 = s[5] - l20 * l20 - l21 * l21;
    const double l22 = sqrt(p2);
    if (!(p0 > 0.0) || !(p1 > 0.0) || !(p2 > 0.0) || !isfinite(p0) || !isfinite(p1) || !isfinite(p2)) status = 3;
    else {
      const double y0 = s[6] / l00, y1 = (s[7] - l10 * y0) / l11, y2 = (s[8] - l20 * y0 - l21 * y1) / l22;
      X[2] = y2 / l22; X[1] = (y1 - l21 * X[2]) / l11; X[0] = (y0 - l10 * X[1] - l20 * X[2]) / l00;
    }
  }
  return status;
}

// Step 5, the gate on the point X of a track whose status is 0 so far: every observation in front of its camera, mean squared pixel error
// below the bound.  Returns the status 0, 4 or 5 and the mean.
template <int G>
__device__ __forceinline__ int tri_gate(const TriArgs& a, const TriTrack& tk, int l, int lane_in_wave, const double* X, int n, double& mean) {
  const uint64_t ob = tk.ob;
  const uint32_t len = tk.len;
  double err = 0.0;
  bool behind = false;
  for (uint32_t k = l; k < len; k += G) {
    const double* cam = a.cams + (uint64_t)GSFM_TRI_CAM_DOUBLES * a.obs_cam[ob + k];
    if (cam[15] == 0.0) continue;
    const double2 xy = a.obs_xy[ob + k];
    const double v0 = X[0] - cam[9], v1 = X[1] - cam[10], v2 = X[2] - cam[11];
    const double px = cam[0] * v0 + cam[1] * v1 + cam[2] * v2, py = cam[3] * v0 + cam[4] * v1 + cam[5] * v2, pz = cam[6] * v0 + cam[7] * v1 + cam[8] * v2;
    behind |= pz < 0.0;
    const double ex = cam[12] * px / pz + cam[13] - xy.x, ey = cam[12] * py / pz + cam[14] - xy.y;
    err += ex * ex + ey * ey;
  }
  mean = tri_group_allsum<G>(err) / (double)n;
  if (tri_group_any<G>(behind, lane_in_wave)) return 4;
  return mean < a.max_sq_err ? 0 : 5;
}

template <int G>
__global__ void __launch_bounds__(G == 64 ? 64 : GSFM_TRI_BLOCK) k_tri_tracks(TriArgs a) {
  constexpr int BLOCK = G == 64 ? 64 : GSFM_TRI_BLOCK;
  constexpr int GROUPS = BLOCK / G;
  constexpr int CAP = G == 4 ? GSFM_TRI_LEN_G4 : GSFM_TRI_LEN_G16;
  __shared__ double lds_rays[G == 64 ? 1 : 3 * GROUPS * CAP];
  const int group = threadIdx.x / G, l = threadIdx.x % G, lane_in_wave = threadIdx.x & 63;
  const TriTrack tk = tri_track<G>(a, lds_rays, group);
  double X[3], mean = 0.0;
  int n;
  int status = tri_front<G>(a, tk, l, lane_in_wave, X, n);
  if (status == 0) status = tri_gate<G>(a, tk, l, lane_in_wave, X, n, mean);
  if (tk.live && l == 0) {
    a.point[3 * tk.t] = X[0]; a.point[3 * tk.t + 1] = X[1]; a.point[3 * tk.t + 2] = X[2];
    a.status[tk.t] = status;
    a.n_views[tk.t] = n;
    a.mean_sq_err[tk.t] = mean;
  }
}

}  // namespace gsfm
