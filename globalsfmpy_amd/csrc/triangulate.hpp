// Host side of gsfm_tracks_triangulate (include/gsfm_tracks.h): validation, the lane classes and the launch order inside a class
// (longest track first), one device slab and the launches of triangulate_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
// gsfm_tracks_triangulate_refine (track_refine.hpp) runs through the same function with a TriRefineHook: the same checks, slab and launch
// order, k_tri_refine_tracks in place of k_tri_tracks and four more outputs.
#pragma once
#include "host_common.hpp"
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

  struct Guard {
    hipStream_t s = nullptr; hipEvent_t ev[2] = {}; void* slab = nullptr;
    ~Guard() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); if (slab) (void)hipFree(slab); if (s) (void)hipStreamDestroy(s); }
  } Gd;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up(bytes); return o; };
  const size_t o_ord = take(4 * T), o_ptr = take(8 * (T + 1)), o_cam = take(4 * O), o_xy = take(16 * O), o_rot = take(24 * N), o_pos = take(24 * N),
               o_k = take(24 * N), o_est = take(N), o_rec = take(8 * GSFM_TRI_CAM_DOUBLES * N), o_plane = take(long_class ? 24 * O : 0),
               o_pt = take(24 * T), o_st = take(4 * T), o_nv = take(4 * T), o_err = take(8 * T), o_it = take(rf ? 4 * T : 0), o_term = take(rf ? 4 * T : 0),
               o_c0 = take(rf ? 8 * T : 0), o_c1 = take(rf ? 8 * T : 0), total = off;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b < (double)total * 1.02 + (64u << 20))
    return (gsfm_status)fail(GSFM_ERR_HIP, "not enough free device memory for the track triangulation (" + std::to_string((long long)(total >> 20)) +
                             " MiB needed, " + std::to_string((long long)(free_b >> 20)) + " MiB free)");
  (void)hipGetLastError();
  HIPCHK_S(hipStreamCreateWithFlags(&Gd.s, hipStreamNonBlocking));
  for (hipEvent_t& e : Gd.ev) HIPCHK_S(hipEventCreate(&e));
  if (hipMalloc(&Gd.slab, total) != hipSuccess) { Gd.slab = nullptr; (void)hipGetLastError(); return (gsfm_status)fail(GSFM_ERR_HIP, "allocating the track triangulation's buffers failed"); }
  char* base = (char*)Gd.slab;
  const hipStream_t s = Gd.s;
  HIPCHK_S(hipMemcpyAsync(base + o_ord, order.data(), 4 * T, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_ptr, track_ptr, 8 * (T + 1), hipMemcpyHostToDevice, s));
  if (O > 0) {
    HIPCHK_S(hipMemcpyAsync(base + o_cam, obs_cam, 4 * O, hipMemcpyHostToDevice, s));
    HIPCHK_S(hipMemcpyAsync(base + o_xy, obs_xy, 16 * O, hipMemcpyHostToDevice, s));
  }
  if (N > 0) {
    HIPCHK_S(hipMemcpyAsync(base + o_rot, rot_aa, 24 * N, hipMemcpyHostToDevice, s));
    HIPCHK_S(hipMemcpyAsync(base + o_pos, cam_pos, 24 * N, hipMemcpyHostToDevice, s));
    HIPCHK_S(hipMemcpyAsync(base + o_k, intrinsics, 24 * N, hipMemcpyHostToDevice, s));
    if (cam_estimated) HIPCHK_S(hipMemcpyAsync(base + o_est, cam_estimated, N, hipMemcpyHostToDevice, s));
  }
  TriArgs a{};
  a.track_ptr = (const uint64_t*)(base + o_ptr); a.obs_cam = (const uint32_t*)(base + o_cam); a.obs_xy = (const double2*)(base + o_xy);
  a.cams = (const double*)(base + o_rec); a.plane = (double*)(base + o_plane); a.n_obs = O;
  a.cos_min_angle = cos_min_angle; a.max_sq_err = max_reprojection_error_pixels * max_reprojection_error_pixels;
  a.point = (double*)(base + o_pt); a.status = (int32_t*)(base + o_st); a.n_views = (int32_t*)(base + o_nv); a.mean_sq_err = (double*)(base + o_err);
  HIPCHK_S(hipEventRecord(Gd.ev[0], s));
  if (N > 0)
    hipLaunchKernelGGL(k_tri_cameras, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, n_cams, (const double*)(base + o_rot), (const double*)(base + o_pos),
                       (const double*)(base + o_k), cam_estimated ? (const uint8_t*)(base + o_est) : (const uint8_t*)nullptr, (double*)(base + o_rec));
  TriRefineArgs ra{};
  if (rf) {
    ra = rf->proto;
    ra.iterations = (int32_t*)(base + o_it); ra.termination = (int32_t*)(base + o_term);
    ra.initial_cost = (double*)(base + o_c0); ra.final_cost = (double*)(base + o_c1);
  }
  auto launch = [&](int c, auto kernel, auto refine_kernel, unsigned groups_per_block, unsigned block) {
    a.n_slots = cb[c + 1] - cb[c];
    if (a.n_slots == 0) return;
    a.order = (const uint32_t*)(base + o_ord) + cb[c];
    const dim3 grid((unsigned)((a.n_slots + groups_per_block - 1) / groups_per_block));
    if (rf) { ra.tri = a; hipLaunchKernelGGL(refine_kernel, grid, dim3(block), 0, s, ra); }
    else hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, a);
  };
  launch(2, k_tri_tracks<64>, k_tri_refine_tracks<64>, 1, 64);   // the long tracks start first
  launch(1, k_tri_tracks<16>, k_tri_refine_tracks<16>, GSFM_TRI_BLOCK / 16, GSFM_TRI_BLOCK);
  launch(0, k_tri_tracks<4>, k_tri_refine_tracks<4>, GSFM_TRI_BLOCK / 4, GSFM_TRI_BLOCK);
  HIPCHK_S(hipEventRecord(Gd.ev[1], s));
  HIPCHK_S(hipMemcpyAsync(point_out, base + o_pt, 24 * T, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipMemcpyAsync(status_out, base + o_st, 4 * T, hipMemcpyDeviceToHost, s));
  if (n_views_out) HIPCHK_S(hipMemcpyAsync(n_views_out, base + o_nv, 4 * T, hipMemcpyDeviceToHost, s));
  if (mean_sq_err_out) HIPCHK_S(hipMemcpyAsync(mean_sq_err_out, base + o_err, 8 * T, hipMemcpyDeviceToHost, s));
  if (rf) {
    if (rf->iterations_out) HIPCHK_S(hipMemcpyAsync(rf->iterations_out, base + o_it, 4 * T, hipMemcpyDeviceToHost, s));
    if (rf->termination_out) HIPCHK_S(hipMemcpyAsync(rf->termination_out, base + o_term, 4 * T, hipMemcpyDeviceToHost, s));
    if (rf->initial_cost_out) HIPCHK_S(hipMemcpyAsync(rf->initial_cost_out, base + o_c0, 8 * T, hipMemcpyDeviceToHost, s));
    if (rf->final_cost_out) HIPCHK_S(hipMemcpyAsync(rf->final_cost_out, base + o_c1, 8 * T, hipMemcpyDeviceToHost, s));
  }
  HIPCHK_S(hipStreamSynchronize(s));
  HIPCHK_S(hipGetLastError());
  if (counts_out) for (size_t t = 0; t < T; ++t) if (status_out[t] >= 0 && status_out[t] < n_status) ++counts_out[status_out[t]];
  if (kernel_ms) { float ms = 0; (void)hipEventElapsedTime(&ms, Gd.ev[0], Gd.ev[1]); *kernel_ms = ms; }
  return GSFM_OK;
}

}  // namespace
