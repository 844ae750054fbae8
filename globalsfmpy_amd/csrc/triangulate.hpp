// Host side of gsfm_tracks_triangulate (include/gsfm_tracks.h): its checks around those of the track arrays, the launch order, the scene in
// one device slab and the launcher over the lane classes (all track_scene.hpp), and the launches of triangulate_kernels.hpp.  Part of
// libgsfm_rot.so's one translation unit.
// gsfm_tracks_triangulate_refine (track_refine.hpp) runs through the same function with a TriRefineHook: the same checks, slab and launch
// order, k_tri_refine_tracks in place of k_tri_tracks and four more outputs.
#pragma once
#include "track_scene.hpp"
#include "track_refine_kernels.hpp"

namespace {

// What gsfm_tracks_triangulate_refine adds to a call: the kernel's options and loss leaf (proto: its TriArgs and output pointers are filled
// here) and the host outputs (each may be NULL).  With a hook the statuses run to 6 and counts_out holds 7 entries.
struct TriRefineHook {
  gsfm::TriRefineArgs proto;
  int32_t *iterations_out, *termination_out;
  double *initial_cost_out, *final_cost_out;
};

gsfm_status tri_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated,
                     uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                     double min_triangulation_angle_degrees, double max_reprojection_error_pixels, double* point_out, int32_t* status_out,
                     int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms, const TriRefineHook* rf = nullptr) {
  const int n_status = rf ? 7 : 6;
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < n_status; ++k) counts_out[k] = 0;
  if (int st = gate_bound_check(min_triangulation_angle_degrees, "min_triangulation_angle_degrees")) return (gsfm_status)st;
  if (int st = gate_bound_check(max_reprojection_error_pixels, "max_reprojection_error_pixels")) return (gsfm_status)st;
  if (n_tracks == 0) return GSFM_OK;   // nothing to triangulate
  if (!point_out || !status_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_cams > 0 && (!rot_aa || !cam_pos || !intrinsics)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = track_arrays_check(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, TrackLimit::tracks_and_lengths, 0, "NULL argument")) return (gsfm_status)st;
  if (const char* why = no_device_reason("the track triangulation")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  const size_t T = n_tracks;
  hvec<uint32_t> order(T);
  uint64_t cb[4];
  tri_bucket(T, track_ptr, order.data(), cb);
  FlatLayout L;
  TrackScene sc;
  sc.take(L, T, T, n_cams, track_ptr[T], cb[3] > cb[2]);
  const auto s_it = L.take<int32_t>(rf ? T : 0), s_term = L.take<int32_t>(rf ? T : 0); const auto s_c0 = L.take<double>(rf ? T : 0), s_c1 = L.take<double>(rf ? T : 0);
  FlatCall fc;
  if (int st = fc.commit(L, "the track triangulation", 1)) return (gsfm_status)st;
  if (int st = sc.upload(fc, order.data(), track_ptr, obs_cam, obs_xy, rot_aa, cam_pos, intrinsics, cam_estimated)) return (gsfm_status)st;
  TriRefineArgs ra{};
  if (rf) {
    ra = rf->proto;
    ra.iterations = fc.ptr(s_it); ra.termination = fc.ptr(s_term); ra.initial_cost = fc.ptr(s_c0); ra.final_cost = fc.ptr(s_c1);
  }
  TriArgs& a = ra.tri;
  HIPCHK_S(fc.begin_span());
  sc.start(fc, cam_estimated != nullptr, min_triangulation_angle_degrees, max_reprojection_error_pixels, &a);
  for_lane_classes(cb, [&](auto G, uint64_t n_slots, uint64_t offset, dim3 grid, dim3 block) {
    a.n_slots = n_slots; a.order = fc.ptr(sc.s_ord) + offset;
    if (!rf) hipLaunchKernelGGL(k_tri_tracks<G()>, grid, block, 0, fc.s, a);
    else hipLaunchKernelGGL(k_tri_refine_tracks<G()>, grid, block, 0, fc.s, ra);
  });
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(point_out, sc.s_pt, 3 * T));
  HIPCHK_S(fc.download(status_out, sc.s_st, T));
  if (n_views_out) HIPCHK_S(fc.download(n_views_out, sc.s_nv, T));
  if (mean_sq_err_out) HIPCHK_S(fc.download(mean_sq_err_out, sc.s_err, T));
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
