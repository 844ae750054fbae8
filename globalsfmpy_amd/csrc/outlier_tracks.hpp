// Host side of gsfm_tracks_outlier_tracks (include/gsfm_tracks.h): the checks of gsfm_tracks_triangulate plus its own, the launch order of
// tri_bucket (triangulate.hpp) filtered to the tracks that are estimated on input with the class slices kept, one device slab
// (flat_call.hpp) and the launches of outlier_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "triangulate.hpp"
#include "outlier_kernels.hpp"

namespace {

gsfm_status outlier_tracks_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated,
                                uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const double* points,
                                const uint8_t* point_estimated, double max_reprojection_error_pixels, double min_triangulation_angle_degrees,
                                int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < 5; ++k) counts_out[k] = 0;
  if (!(max_reprojection_error_pixels >= 0.0) || !std::isfinite(max_reprojection_error_pixels))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "max_reprojection_error_pixels must be finite and not negative");
  if (!(min_triangulation_angle_degrees >= 0.0) || !std::isfinite(min_triangulation_angle_degrees))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "min_triangulation_angle_degrees must be finite and not negative");
  if (n_tracks == 0) return GSFM_OK;   // nothing to examine
  if (!track_ptr || !points || !status_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
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

  // the launch order of the triangulation without the tracks that are not estimated: those are status 1 and are not launched
  hvec<uint32_t> order(T);
  uint64_t all[4], cb[4] = {0, 0, 0, 0};
  tri_bucket(T, track_ptr, order.data(), all);
  size_t E = 0;
  for (int c = 0; c < 3; ++c) {
    for (uint64_t k = all[c]; k < all[c + 1]; ++k)
      if (!point_estimated || point_estimated[order[k]]) order[E++] = order[k];
    cb[c + 1] = E;
  }
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

  const bool long_class = cb[3] > cb[2];
  FlatLayout L;
  const auto s_ord = L.take<uint32_t>(E); const auto s_ptr = L.take<uint64_t>(T + 1); const auto s_cam = L.take<uint32_t>(O); const auto s_xy = L.take<double2>(O);
  const auto s_rot = L.take<double>(3 * N), s_pos = L.take<double>(3 * N), s_k = L.take<double>(3 * N); const auto s_est = L.take<uint8_t>(N);
  const auto s_rec = L.take<double>(GSFM_TRI_CAM_DOUBLES * N), s_plane = L.take<double>(long_class ? 3 * O : 0), s_pt = L.take<double>(3 * T);
  const auto s_st = L.take<int32_t>(T), s_nv = L.take<int32_t>(T); const auto s_err = L.take<double>(T);
  FlatCall fc;
  if (int st = fc.commit(L, "the outlier rule", 1)) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  HIPCHK_S(fc.upload(s_ord, order.data(), E));
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
  HIPCHK_S(fc.upload(s_pt, points, 3 * T));
  HIPCHK_S(fc.upload(s_st, status.data(), T));   // 1 where the kernels do not write
  HIPCHK_S(fc.zero(s_nv, T));
  HIPCHK_S(fc.zero(s_err, T));
  OutlierArgs oa{};
  TriArgs& a = oa.tri;
  a.track_ptr = fc.ptr(s_ptr); a.obs_cam = fc.ptr(s_cam); a.obs_xy = fc.ptr(s_xy);
  a.cams = fc.ptr(s_rec); a.plane = fc.ptr(s_plane); a.n_obs = O;
  a.cos_min_angle = std::cos(min_triangulation_angle_degrees * M_PI / 180.0);
  a.max_sq_err = max_reprojection_error_pixels * max_reprojection_error_pixels;
  a.point = nullptr; a.status = fc.ptr(s_st); a.n_views = fc.ptr(s_nv); a.mean_sq_err = fc.ptr(s_err);
  oa.points = fc.ptr(s_pt);
  HIPCHK_S(fc.begin_span());
  if (N > 0)
    hipLaunchKernelGGL(k_tri_cameras, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, n_cams, (const double*)fc.ptr(s_rot), (const double*)fc.ptr(s_pos),
                       (const double*)fc.ptr(s_k), cam_estimated ? (const uint8_t*)fc.ptr(s_est) : (const uint8_t*)nullptr, fc.ptr(s_rec));
  auto launch = [&](int c, auto kernel, unsigned groups_per_block, unsigned block) {
    a.n_slots = cb[c + 1] - cb[c];
    if (a.n_slots == 0) return;
    a.order = fc.ptr(s_ord) + cb[c];
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.n_slots + groups_per_block - 1) / groups_per_block)), dim3(block), 0, s, oa);
  };
  launch(2, k_outlier_tracks<64>, 1, 64);   // the long tracks start first
  launch(1, k_outlier_tracks<16>, GSFM_TRI_BLOCK / 16, GSFM_TRI_BLOCK);
  launch(0, k_outlier_tracks<4>, GSFM_TRI_BLOCK / 4, GSFM_TRI_BLOCK);
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(status_out, s_st, T));
  if (n_views_out) HIPCHK_S(fc.download(n_views_out, s_nv, T));
  if (mean_sq_err_out) HIPCHK_S(fc.download(mean_sq_err_out, s_err, T));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  return finish();
}

}  // namespace
