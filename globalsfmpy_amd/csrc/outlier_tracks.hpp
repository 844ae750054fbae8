// Host side of gsfm_tracks_outlier_tracks (include/gsfm_tracks.h): its checks around those of the track arrays, the launch order without the
// tracks that are not estimated on input, the scene in one device slab and the launcher over the lane classes (all track_scene.hpp), and the
// launches of outlier_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "track_scene.hpp"
#include "outlier_kernels.hpp"

namespace {

gsfm_status outlier_tracks_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated,
                                uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const double* points,
                                const uint8_t* point_estimated, double max_reprojection_error_pixels, double min_triangulation_angle_degrees,
                                int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < 5; ++k) counts_out[k] = 0;
  if (int st = gate_bound_check(max_reprojection_error_pixels, "max_reprojection_error_pixels")) return (gsfm_status)st;
  if (int st = gate_bound_check(min_triangulation_angle_degrees, "min_triangulation_angle_degrees")) return (gsfm_status)st;
  if (n_tracks == 0) return GSFM_OK;   // nothing to examine
  if (!points || !status_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_cams > 0 && (!rot_aa || !cam_pos || !intrinsics)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = track_arrays_check(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, TrackLimit::tracks_and_lengths, 0, "NULL argument")) return (gsfm_status)st;

  // the launch order of the triangulation without the tracks that are not estimated: those are status 1 and are not launched
  const size_t T = n_tracks;
  hvec<uint32_t> order(T);
  uint64_t all[4], cb[4];
  tri_bucket(T, track_ptr, order.data(), all);
  const size_t E = tri_keep_estimated(order.data(), all, point_estimated, cb);
  hvec<int32_t> status(T);
  for (size_t t = 0; t < T; ++t) status[t] = (!point_estimated || point_estimated[t]) ? 0 : 1;
  auto finish = [&]() {
    if (counts_out) for (size_t t = 0; t < T; ++t) if (status_out[t] >= 0 && status_out[t] < 5) ++counts_out[status_out[t]];
    return GSFM_OK;
  };
  if (E == 0) {   // no track is estimated: nothing for the device
    for (size_t t = 0; t < T; ++t) {
      status_out[t] = 1;
      if (n_views_out) n_views_out[t] = 0;
      if (mean_sq_err_out) mean_sq_err_out[t] = 0.0;
    }
    return finish();
  }
  if (const char* why = no_device_reason("the outlier rule")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  FlatLayout L;
  TrackScene sc;
  sc.take(L, E, T, n_cams, track_ptr[T], cb[3] > cb[2]);
  FlatCall fc;
  if (int st = fc.commit(L, "the outlier rule", 1)) return (gsfm_status)st;
  if (int st = sc.upload(fc, order.data(), track_ptr, obs_cam, obs_xy, rot_aa, cam_pos, intrinsics, cam_estimated)) return (gsfm_status)st;
  HIPCHK_S(fc.upload(sc.s_pt, points, 3 * T));
  HIPCHK_S(fc.upload(sc.s_st, status.data(), T));   // 1 where the kernels do not write
  HIPCHK_S(fc.zero(sc.s_nv, T));
  HIPCHK_S(fc.zero(sc.s_err, T));
  OutlierArgs oa{};
  TriArgs& a = oa.tri;
  HIPCHK_S(fc.begin_span());
  sc.start(fc, cam_estimated != nullptr, min_triangulation_angle_degrees, max_reprojection_error_pixels, &a);
  a.point = nullptr; oa.points = fc.ptr(sc.s_pt);   // (the points are an input here)
  for_lane_classes(cb, [&](auto G, uint64_t n_slots, uint64_t offset, dim3 grid, dim3 block) {
    a.n_slots = n_slots; a.order = fc.ptr(sc.s_ord) + offset;
    hipLaunchKernelGGL(k_outlier_tracks<G()>, grid, block, 0, fc.s, oa);
  });
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(status_out, sc.s_st, T));
  if (n_views_out) HIPCHK_S(fc.download(n_views_out, sc.s_nv, T));
  if (mean_sq_err_out) HIPCHK_S(fc.download(mean_sq_err_out, sc.s_err, T));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  return finish();
}

}  // namespace
