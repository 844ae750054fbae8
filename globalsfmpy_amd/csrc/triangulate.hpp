// Host side of gsfm_tracks_triangulate (include/gsfm_tracks.h): validation, the lane classes and the launch order inside a class
// (longest track first), one device slab (flat_call.hpp) and the launches of triangulate_kernels.hpp.  Part of libgsfm_rot.so's one
// translation unit.
// gsfm_tracks_triangulate_refine (track_refine.hpp) runs through the same function with a TriRefineHook: the same checks, slab and launch
// order, k_tri_refine_tracks in place of k_tri_tracks and four more outputs.
#pragma once
#include "flat_call.hpp"
#include "triangulate_kernels.hpp"
#include "track_refine_kernels.hpp"
#include "../../include/gsfm_tracks.h"

namespace {

// 0, 1, 2: groups of 4, 16, 64 lanes -- a function of the track's length alone (include/gsfm_tracks.h)
inline int tri_class_of(uint64_t len) { return len <= GSFM_TRI_LEN_G4 ? 0 : len <= GSFM_TRI_LEN_G16 ? 1 : 2; }

// The launch order: the tracks of class 0, then 1, then 2; inside a class by descending length, equal lengths by track index.
// class_begin[c] .. class_begin[c + 1] is class c's slice of `order`.
void tri_bucket(uint64_t n_tracks, const uint64_t* track_ptr, uint32_t* order, uint64_t class_begin[4]) {
  uint64_t count[3] = {0, 0, 0};
  for (uint64_t t = 0; t < n_tracks; ++t) ++count[tri_class_of(track_ptr[t + 1] - track_ptr[t])];
  class_begin[0] = 0;
  for (int c = 0; c < 3; ++c) class_begin[c + 1] = class_begin[c] + count[c];
  uint64_t cursor[3] = {class_begin[0], class_begin[1], class_begin[2]};
  for (uint64_t t = 0; t < n_tracks; ++t) order[cursor[tri_class_of(track_ptr[t + 1] - track_ptr[t])]++] = (uint32_t)t;
  for (int c = 0; c < 3; ++c)
    std::stable_sort(order + class_begin[c], order + class_begin[c + 1], [track_ptr](uint32_t x, uint32_t y) {
      return track_ptr[x + 1] - track_ptr[x] > track_ptr[y + 1] - track_ptr[y];
    });
}

// What gsfm_tracks_triangulate_refine adds to a call: the kernel's options and loss leaf (proto: its TriArgs and output pointers are filled
// here) and the host outputs (each may be NULL).  With a hook the statuses run to 6 and counts_out holds 7 entries.
struct TriRefineHook {
  gsfm::TriRefineArgs proto;
  int32_t* iterations_out;
  int32_t* termination_out;
  double* initial_cost_out;
  double* final_cost_out;
};

gsfm_status tri_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated,
                     uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                     double min_triangulation_angle_degrees, double max_reprojection_error_pixels, double* point_out, int32_t* status_out,
                     int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms, const TriRefineHook* rf = nullptr) {
  const int n_status = rf ? 7 : 6;
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < n_status; ++k) counts_out[k] = 0;
  if (!(min_triangulation_angle_degrees >= 0.0) || !std::isfinite(min_triangulation_angle_degrees))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "min_triangulation_angle_degrees must be finite and not negative");
  if (!(max_reprojection_error_pixels >= 0.0) || !std::isfinite(max_reprojection_error_pixels))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "max_reprojection_error_pixels must be finite and not negative");
  if (n_tracks == 0) return GSFM_OK;   // nothing to triangulate
  if (!track_ptr || !point_out || !status_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_cams > 0 && (!rot_aa || !cam_pos || !intrinsics)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_tracks >= (1ull << 31)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 tracks)");
  if (track_ptr[0] != 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "track_ptr[0] must be 0");
  for (uint64_t t = 0; t < n_tracks; ++t) {
    if (track_ptr[t + 1] < track_ptr[t]) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "track_ptr decreases at track " + std::to_string(t));
    if (track_ptr[t + 1] - track_ptr[t] >= (1ull << 31)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "track " + std::to_string(t) + " is too long (2^31 observations)");
  }
  const size_t T = n_tracks, N = n_cams, O = track_ptr[T];
  if (O > 0 && (!obs_cam || !obs_xy)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  for (size_t k = track_ptr[0]; k < O; ++k)
    if (obs_cam[k] >= n_cams) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "observation " + std::to_string(k) + " has an out-of-range camera index");
  if (const char* why = no_device_reason("the track triangulation")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  hvec<uint32_t> order(T);
  uint64_t cb[4];
  tri_bucket(T, track_ptr, order.data(), cb);
  const bool long_class = cb[3] > cb[2];
  const double cos_min_angle = std::cos(min_triangulation_angle_degrees * M_PI / 180.0);

  FlatLayout L;
  const auto s_ord = L.take<uint32_t>(T); const auto s_ptr = L.take<uint64_t>(T + 1); const auto s_cam = L.take<uint32_t>(O); const auto s_xy = L.take<double2>(O);
  const auto s_rot = L.take<double>(3 * N), s_pos = L.take<double>(3 * N), s_k = L.take<double>(3 * N); const auto s_est = L.take<uint8_t>(N);
  const auto s_rec = L.take<double>(GSFM_TRI_CAM_DOUBLES * N), s_plane = L.take<double>(long_class ? 3 * O : 0), s_pt = L.take<double>(3 * T);
  const auto s_st = L.take<int32_t>(T), s_nv = L.take<int32_t>(T); const auto s_err = L.take<double>(T);
  const auto s_it = L.take<int32_t>(rf ? T : 0), s_term = L.take<int32_t>(rf ? T : 0); const auto s_c0 = L.take<double>(rf ? T : 0), s_c1 = L.take<double>(rf ? T : 0);
  FlatCall fc;
  if (int st = fc.commit(L, "the track triangulation", 1)) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  HIPCHK_S(fc.upload(s_ord, order.data(), T));
  HIPCHK_S(fc.upload(s_ptr, track_ptr, T + 1));
  if (O > 0) {
    HIPCHK_S(fc.upload(s_cam, obs_cam, O));
    HIPCHK_S(fc.upload(s_xy, obs_xy, O));
  }
  if (N > 0) {
    HIPCHK_S(fc.upload(s_rot, rot_aa, 3 * N));
    HIPCHK_S(fc.upload(s_pos, cam_pos, 3 * N));
    HIPCHK_S(fc.upload(s_k, intrinsics, 3 * N));
    if (cam_estimated) HIPCHK_S(fc.upload(s_est, cam_estimated, N));
  }
  TriArgs a{};
  a.track_ptr = fc.ptr(s_ptr); a.obs_cam = fc.ptr(s_cam); a.obs_xy = fc.ptr(s_xy);
  a.cams = fc.ptr(s_rec); a.plane = fc.ptr(s_plane); a.n_obs = O;
  a.cos_min_angle = cos_min_angle; a.max_sq_err = max_reprojection_error_pixels * max_reprojection_error_pixels;
  a.point = fc.ptr(s_pt); a.status = fc.ptr(s_st); a.n_views = fc.ptr(s_nv); a.mean_sq_err = fc.ptr(s_err);
  HIPCHK_S(fc.begin_span());
  if (N > 0)
    hipLaunchKernelGGL(k_tri_cameras, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, n_cams, (const double*)fc.ptr(s_rot), (const double*)fc.ptr(s_pos),
                       (const double*)fc.ptr(s_k), cam_estimated ? (const uint8_t*)fc.ptr(s_est) : (const uint8_t*)nullptr, fc.ptr(s_rec));
  TriRefineArgs ra{};
  if (rf) {
    ra = rf->proto;
    ra.iterations = fc.ptr(s_it); ra.termination = fc.ptr(s_term); ra.initial_cost = fc.ptr(s_c0); ra.final_cost = fc.ptr(s_c1);
  }
  auto launch = [&](int c, auto kernel, auto refine_kernel, unsigned groups_per_block, unsigned block) {
    a.n_slots = cb[c + 1] - cb[c];
    if (a.n_slots == 0) return;
    a.order = fc.ptr(s_ord) + cb[c];
    const dim3 grid((unsigned)((a.n_slots + groups_per_block - 1) / groups_per_block));
    if (rf) { ra.tri = a; hipLaunchKernelGGL(refine_kernel, grid, dim3(block), 0, s, ra); }
    else hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, a);
  };
  launch(2, k_tri_tracks<64>, k_tri_refine_tracks<64>, 1, 64);   // the long tracks start first
  launch(1, k_tri_tracks<16>, k_tri_refine_tracks<16>, GSFM_TRI_BLOCK / 16, GSFM_TRI_BLOCK);
  launch(0, k_tri_tracks<4>, k_tri_refine_tracks<4>, GSFM_TRI_BLOCK / 4, GSFM_TRI_BLOCK);
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(point_out, s_pt, 3 * T));
  HIPCHK_S(fc.download(status_out, s_st, T));
  if (n_views_out) HIPCHK_S(fc.download(n_views_out, s_nv, T));
  if (mean_sq_err_out) HIPCHK_S(fc.download(mean_sq_err_out, s_err, T));
  if (rf) {
    if (rf->iterations_out) HIPCHK_S(fc.download(rf->iterations_out, s_it, T));
    if (rf->termination_out) HIPCHK_S(fc.download(rf->termination_out, s_term, T));
    if (rf->initial_cost_out) HIPCHK_S(fc.download(rf->initial_cost_out, s_c0, T));
    if (rf->final_cost_out) HIPCHK_S(fc.download(rf->final_cost_out, s_c1, T));
  }
  HIPCHK_S(fc.sync());
  if (counts_out) for (size_t t = 0; t < T; ++t) if (status_out[t] >= 0 && status_out[t] < n_status) ++counts_out[status_out[t]];
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  return GSFM_OK;
}

}  // namespace
