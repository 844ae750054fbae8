// Host side of gsfm_tracks_triangulate_refine (include/gsfm_tracks.h): the checks of the options, the loss leaf the kernel takes
// (track_scene.hpp's one_leaf_loss), and the call of tri_impl (triangulate.hpp) with the refinement hook -- its validation, slab and launch
// order serve both entries.
// Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "triangulate.hpp"

namespace {

gsfm_status tri_refine_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated,
                            uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                            double min_triangulation_angle_degrees, double max_reprojection_error_pixels, const gsfm_tracks_refine_options* options,
                            const gsfm_loss_node* loss, int32_t n_loss_nodes, double* point_out, int32_t* status_out, int32_t* n_views_out,
                            double* mean_sq_err_out, int32_t* iterations_out, double* initial_cost_out, double* final_cost_out,
                            int32_t* termination_out, uint64_t* counts_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < 7; ++k) counts_out[k] = 0;
  gsfm_tracks_refine_options o;
  gsfm_tracks_refine_default_options(&o);
  if (options) o = *options;
  TriRefineHook rf{};
  if (int st = one_leaf_loss(loss, n_loss_nodes, "track refinement", &rf.proto.leaf)) return (gsfm_status)st;   // (its node count before a NULL program)
  auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!(o.function_tolerance >= 0.0) || !(o.gradient_tolerance >= 0.0) || !(o.parameter_tolerance >= 0.0) || !std::isfinite(o.function_tolerance) ||
      !std::isfinite(o.gradient_tolerance) || !std::isfinite(o.parameter_tolerance) || !std::isfinite(o.min_relative_decrease))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the refinement's tolerances must be finite and not negative");
  if (!positive(o.initial_trust_region_radius) || !positive(o.max_trust_region_radius) || !(o.min_trust_region_radius >= 0.0) || !std::isfinite(o.min_trust_region_radius))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the refinement's trust-region radii must be finite and positive");
  if (!o.refine)   // the entry without the refinement (no hook below): k_tri_tracks and its bytes; a status 6 cannot occur
    for (uint64_t t = 0; t < n_tracks; ++t) {
      if (iterations_out) iterations_out[t] = 0;
      if (termination_out) termination_out[t] = -1;
      if (initial_cost_out) initial_cost_out[t] = 0.0;
      if (final_cost_out) final_cost_out[t] = 0.0;
    }
  rf.proto.max_num_iterations = std::min(std::max(o.max_num_iterations, 0), GSFM_TRR_MAX_ITERATIONS);
  rf.proto.function_tolerance = o.function_tolerance; rf.proto.gradient_tolerance = o.gradient_tolerance;
  rf.proto.parameter_tolerance = o.parameter_tolerance; rf.proto.min_relative_decrease = o.min_relative_decrease;
  rf.proto.initial_radius = o.initial_trust_region_radius; rf.proto.max_radius = o.max_trust_region_radius; rf.proto.min_radius = o.min_trust_region_radius;
  rf.iterations_out = iterations_out; rf.termination_out = termination_out; rf.initial_cost_out = initial_cost_out; rf.final_cost_out = final_cost_out;
  return tri_impl(n_cams, rot_aa, cam_pos, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy, min_triangulation_angle_degrees,
                  max_reprojection_error_pixels, point_out, status_out, n_views_out, mean_sq_err_out, counts_out, kernel_ms, o.refine ? &rf : nullptr);
}

}  // namespace
