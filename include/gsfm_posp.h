/* gsfm_posp.h -- C ABI of camera-position estimation with point-to-camera constraints on the GPU (libgsfm_rot.so).
 *
 * Restates the reference's GSfMNonlinearPositionEstimator::EstimatePositions with min_num_points_per_view > 0
 * (src/GSfM_nonlinear_position_estimator.cpp: AddCameraToCameraConstraints + AddPointToCameraConstraints / AddTrackToProblem): the
 * camera-to-camera problem of gsfm_pos.h plus, per chosen feature track, one 3D point tied to every camera that observes it.  gsfm_pos.h
 * and its ABI version are unchanged; the track arrays are those of gsfm_tracks.h.
 *
 * Unknowns.  One 3-vector per camera and per point, cameras first: one array of (n_cams + n_tracks) x 3.
 *
 * Camera-to-camera residual.  gsfm_pos.h's, by the same device routine: r = (c_j - c_i) / n - R(aa_i)^T t_ij, n = |c_j - c_i|,
 * n := 1 below 1e-12, weight 1.
 *
 * Point-to-camera residual.  For a used observation o of camera k (centre c_k) and point X_t (Theia's PairwiseTranslationError between a
 * camera centre and a point, as AddTrackToProblem adds it):
 *   r_o = w_p ((X_t - c_k) / n - ray_o),  n = |X_t - c_k| with the same guard;
 *   d r_o / d X_t = w_p (I - u u^T) / n  (w_p I in the guard branch),  d r_o / d c_k = its negative;
 *   w_p > 0 is one scalar per problem (point_to_camera_weight).
 *   ray_o = normalise(R(aa_k)^T ((x - u) / f, (y - v) / f, 1)), computed on the device once, at create, with R = Ceres'
 *   AngleAxisToRotationMatrix (the routine of the edge directions), (f, u, v) the intrinsics triple of gsfm_tracks.h and aa_k from
 *   ray_rot_aa, an array of its own (the estimator layer may rotate rays by other orientations than the edges': see
 *   include/gsfm/GSfM_nonlinear_position_estimator.hpp).
 *
 * Loss.  The problem's ONE loss applies to both residual kinds through Ceres' Corrector on s = |r|^2 (for an observation the weighted
 * residual's), as the reference hands the same loss object to both.  gsfm_posp_set_loss takes what gsfm_pos_set_loss takes (the in-kernel
 * leaves and programs).  A host-callback loss is refused (gsfm_posp_set_loss_callback: GSFM_ERR_INVALID_ARG before any device call).
 *
 * Used observations, active nodes.
 *   A camera is a parameter when it appears in an edge (gsfm_pos.h's rule).  A camera-side observation is one whose camera is such a camera.
 *   A point is ACTIVE with at least two camera-side observations, and an observation is USED when its camera appears in an edge and its
 *   point is active.  DEPARTURE from the reference, which also adds a point seen once: such a point's Schur contribution
 *   H - H C^-1 H is zero up to the damping, so it constrains nothing; its observation is dropped with it (it would tie a camera to a
 *   point that does not move).
 *   The fixed camera is inactive, but its observations are used: they enter C_t, g_t and the cost; the camera has no column.
 *   Everything inactive passes through a solve bit for bit.
 *
 * LM.  gsfm_pos_solve's rules and gsfm_pos_options, unchanged.  Jacobi scaling covers every camera and point.  With remove_scale_gauge the
 * step loses its component along v = x - c_fixed over all active cameras and points.  dense_max_cams is ignored: every step is solved by
 * the Schur-complement PCG below (with n_tracks = 0 the operator is gsfm_pos.h's PCG operator).
 *
 * Linear solve.  The points are eliminated as in gsfm_ba.h: C~_t = S_t C_t S_t + D^2_t inverted per point (cofactors, and the second tier
 * of gsfm_ba.h for a badly conditioned block).  The normal matrix is a block graph Laplacian over cameras and points: camera blocks
 * sum_edges H_e + B_k with B_k = sum_{o in k} H_o, point blocks C_t = sum_{o in t} H_o, off-diagonal -H_e and -H_o.  The reduced camera
 * operator  Sc = S_c (L_edges + B) S_c + D^2_c - E~ C~^-1 E~^T  is never formed; one product is a point pass and a camera pass that carries
 * the edge Laplacian and the Schur term together.  PCG from zero until sqrt(r.M^-1 r / b.M^-1 b) <= cg_relative_tolerance, with
 * cg_stall_iterations and cg_check_interval as in gsfm_pos.h; a r.M^-1 r that is not positive ends the solve as stalled (gsfm_ba.h's
 * rule: points are eliminated here too).  Preconditioner: the block diagonal of Sc, sum_edges H_e + sum_obs (H_o - H_o G_t H_o), scaled and
 * damped, inverted per camera.  The points follow by back-substitution.  A dense Schur complement is not part of this library.
 *
 * Order of the sums (part of the definition).  Per track: the lane groups of gsfm_tracks.h (G = 4 / 16 / 64 by the CSR length, lane l adds
 * the observations l, l + G, ..., then the xor butterfly).  Per camera row: one wavefront strides first the row's edge entries
 * (gsfm_pos.h's order), then its used observations in ascending observation index, then the fixed shuffle tree.  Global sums: 512
 * partials.  The cost is the edge sum plus the track sum.  No atomics: two solves return the same bytes.
 */
#ifndef GSFM_POSP_H_
#define GSFM_POSP_H_

#include <stdint.h>
#include "gsfm_pos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_POSP_ABI_VERSION 1

typedef struct gsfm_posp_problem gsfm_posp_problem;

typedef struct {
  gsfm_pos_summary pos;                /* gsfm_pos.h's fields (num_dense_solves stays 0) */
  uint64_t num_observations_used;
  uint64_t num_active_points;
} gsfm_posp_summary;

int gsfm_posp_abi_version(void);

/* n_cams, edges, rel_t, rot_aa: as gsfm_pos_problem_create.  ray_rot_aa (n_cams x 3) and intrinsics (n_cams x 3: f u v) are read for the
 * cameras of used observations; both may be NULL when n_tracks = 0.  track_ptr (n_tracks + 1), obs_cam, obs_xy: the track CSR of
 * gsfm_tracks.h.  Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: gsfm_pos_problem_create's and
 * gsfm_ba_problem_create's checks, and a point_to_camera_weight that is not finite and positive); without a device GSFM_ERR_NO_DEVICE. */
gsfm_status gsfm_posp_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                     const double* rot_aa, const double* ray_rot_aa, const double* intrinsics, uint64_t n_tracks,
                                     const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, double point_to_camera_weight,
                                     gsfm_posp_problem** out);
gsfm_status gsfm_posp_set_loss(gsfm_posp_problem* p, const gsfm_loss_node* program, int32_t n_nodes);   /* n_nodes = 0: Ceres' NULL loss */
/* always refused with GSFM_ERR_INVALID_ARG, before any device call: a host-callback loss is not supported here */
gsfm_status gsfm_posp_set_loss_callback(gsfm_posp_problem* p, gsfm_loss_callback fn, void* user);
/* cam_pos_inout: n_cams x 3, point_inout: n_tracks x 3 (may be NULL when n_tracks = 0): start values in, estimates out (active nodes only
 * are written).  fixed_cam: the camera held constant (must appear in an edge), or -1.  options / summary may be NULL. */
gsfm_status gsfm_posp_solve(gsfm_posp_problem* p, double* cam_pos_inout, double* point_inout, int32_t fixed_cam, const gsfm_pos_options* options,
                            gsfm_posp_summary* summary);

/* ---- checks of the solve's own code (the tests compare them with a high-precision reference); every output may be NULL ---- */
/* r_edge_out n_edges x 3, rho_edge_out n_edges; r_obs_out n_obs x 3 (the weighted residual), rho_obs_out n_obs, ray_out n_obs x 3; zeros
 * for an observation that is not used */
gsfm_status gsfm_posp_residuals(gsfm_posp_problem* p, const double* cam_pos, const double* points, double* r_edge_out, double* rho_edge_out,
                                double* r_obs_out, double* rho_obs_out, double* ray_out);
/* cost, gradient (n_cams x 3, n_tracks x 3) and the diagonal blocks (n_cams x 9: sum_edges H_e + B_k; n_tracks x 9: C_t; row-major) at the
 * point given, every present camera active (as gsfm_pos_linearize).  The blocks stay on the device for gsfm_posp_schur_matvec. */
gsfm_status gsfm_posp_linearize(gsfm_posp_problem* p, const double* cam_pos, const double* points, double* cost, double* grad_cam,
                                double* grad_point, double* diag_cam, double* diag_point);
/* y = Sc v (n_cams x 3) for the last gsfm_posp_linearize or gsfm_posp_step_check (with that call's active set), with the Jacobi scale of
 * that point (options->jacobi_scaling) and D^2 at `radius`; the identity on inactive cameras. */
gsfm_status gsfm_posp_schur_matvec(gsfm_posp_problem* p, const double* v, double radius, const gsfm_pos_options* options, double* y);
/* One LM step's linear algebra at the point given, exactly as iteration 1 of gsfm_posp_solve computes it but at the given radius (the same
 * code), stopped before the accept / reject decision:
 *   rhs_out (n_cams x 3) the reduced right-hand side;  yc_out (n_cams x 3) the PCG solution;  yp_out (n_tracks x 3) the back-substituted
 *   points;  delta_cam_out / delta_point_out the step -S y after the gauge projection;
 *   scal_out[4]  model cost change, delta.g, delta^T L delta, PCG's final sqrt(r.M^-1 r / b.M^-1 b);   info_out[2]  PCG iterations, stalled (0 / 1) */
gsfm_status gsfm_posp_step_check(gsfm_posp_problem* p, const double* cam_pos, const double* points, int32_t fixed_cam, double radius,
                                 const gsfm_pos_options* options, double* rhs_out, double* yc_out, double* yp_out, double* delta_cam_out,
                                 double* delta_point_out, double* scal_out, int32_t* info_out);
/* Mean device time in microseconds (HIP events, `reps` launches after a warm one) at the point given, damped at `radius`:
 * out_us[7] = rays, track-side linearisation, camera-side linearisation, track cost, point pass, camera pass, preconditioner.
 * For tools/time_position_points.py. */
gsfm_status gsfm_posp_time_kernels(gsfm_posp_problem* p, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us);
void gsfm_posp_problem_destroy(gsfm_posp_problem* p);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_POSP_H_ */
