/* gsfm_ba.h -- C ABI of the bundle adjustment of camera positions and points on the GPU (libgsfm_rot.so).
 *
 * Restates Theia's BundleAdjuster as the reference pipeline calls it right after EstimateStructure():
 * GlobalReconstructionEstimator::BundleAdjustCameraPositionsAndPoints (refine_camera_positions_and_points_after_position_estimation,
 * intrinsics_to_optimize = NONE): every camera's ORIENTATION and intrinsics are held, camera positions and 3D points move.
 *
 * Cameras and tracks are the flat arrays of gsfm_tracks.h: rot_aa (n_cams x 3 angle-axis, world -> camera, R = Ceres'
 * AngleAxisToRotationMatrix), intrinsics (n_cams x 3: f u v), cam_estimated (n_cams bytes, NULL = all estimated), the CSR track_ptr /
 * obs_cam / obs_xy, and point_estimated (n_tracks bytes, NULL = all estimated).
 *
 * Used observations, active nodes.  An observation is USED when its camera and its track are both estimated.  A camera or a point with no
 * used observation is INACTIVE.  Inactive and unestimated cameras and points are no parameters: they pass through a solve bit for bit.
 *
 * Definition.
 *   residual   per used observation of camera k (orientation R, centre o) and point X:  p = R (X - o),
 *              r = (f p_x / p_z + u - x, f p_y / p_z + v - y),  s = |r|^2.
 *   Jacobian   J_point = (f / p_z) [[1, 0, -p_x / p_z], [0, 1, -p_y / p_z]] R  and  J_cam = -J_point  (r depends on X - o alone),
 *              corrected by Ceres' Corrector exactly as in step "residual" of gsfm_tracks_triangulate_refine (the same device routine):
 *              J~ = sqrt(rho') (J - alpha / s r r^T J), r~ = sqrt(rho') / (1 - alpha) r.
 *   cost       1/2 sum rho(s) over the used observations.
 *   normal matrix   with H_e = J~^T J~ (3 x 3) and a_e = J~^T r~ (J~ the corrected POINT Jacobian): camera blocks B_k = sum_{e in k} H_e,
 *              point blocks C_t = sum_{e in t} H_e, off-diagonal blocks -H_e; gradient g_k = -sum_{e in k} a_e, g_t = sum_{e in t} a_e.
 *   LM         the rules gsfm_pos.h restates for gsfm_pos_solve: Ceres 1.14's TrustRegionMinimizer with the LEVENBERG_MARQUARDT
 *              strategy.  Jacobi scaling S = 1 / (1 + sqrt(diag)) per coordinate of every camera and point, from the start point, kept
 *              for the solve; D^2 = clamp(S^2 diag, min_lm_diagonal, max_lm_diagonal) / radius; the step solves
 *              (S L S + D^2) y = S g and is delta = -S y; model cost change -delta.g - delta^T L delta / 2; invalid-step rule (the
 *              fifth in a row fails), accept when cost change / model change > min_relative_decrease, radius rule of
 *              LevenbergMarquardtStrategy; function, gradient (max norm over the active coordinates) and parameter tolerances.
 *   linear solve    the points are eliminated.  In scaled, damped coordinates C~_t = S_t C_t S_t + D^2_t is inverted per point by
 *              cofactors (3 x 3, positive definite by the diagonal clamp).  With E~_e = -S_k H_e S_t the reduced camera system is
 *              Sc y_c = b_c - E~ C~^-1 b_p,  Sc = B~ - E~ C~^-1 E~^T,  solved by preconditioned conjugate gradients from y_c = 0 until
 *              sqrt(r.M^-1 r / b.M^-1 b) <= cg_relative_tolerance.  Sc is never formed: one product is a point pass,
 *              w_t = C~_t^-1 sum_{e in t} E~_e^T v_k(e), then a camera pass, y_k = B~_k v_k - sum_{e in k} E~_e w_t(e).  The
 *              preconditioner M is the block diagonal of Sc, B~_k - sum_{e in k} E~_e C~_t^-1 E~_e^T (Ceres' SCHUR_JACOBI), inverted
 *              per camera.  The points follow by y_p = C~^-1 (b_p - E~^T y_c).
 *   gauge      the cost is invariant under a common translation of all cameras and points and under scaling about any centre; Ceres
 *              and Theia fix nothing and leave these four directions to the damping.  With remove_gauge = 1 (default) each step first
 *              loses its mean over the active nodes, per axis, and then its component along v = x - mean(x) (mean over the active
 *              nodes): delta -= (delta.v / v.v) v.  J v = 0 for all four directions, so the model cost change is unchanged (the
 *              argument of gsfm_pos.h's scale gauge).  remove_gauge = 0 is Ceres' plain step.  Compare results after removing
 *              translation and scale.
 * The loss is ONE leaf of the kinds gsfm_tracks_triangulate_refine accepts (TRIVIAL, HUBER, SOFT_L1, TUKEY, GEMAN_MCCLURE; the pipeline's
 * is HUBER of width 10) or n_nodes = 0, Ceres' NULL loss (the state of a new problem).
 *
 * Order of the sums (part of the definition).  Sums over a track's observations (C_t, g_t, the cost, the point pass) run in the lane
 * groups of gsfm_tracks.h: G = 4 / 16 / 64 by the track's CSR length, lane l adds the observations l, l + G, ... from 0, then the xor
 * butterfly.  Sums over a camera's observations run over its used observations in ascending observation index: lane l of 64 adds the
 * entries l, l + 64, ..., then a shuffle tree (v += v of lane l + offset, offsets 32, 16, ..., 1).  Global sums use 512 partials in a fixed
 * order.  No atomics: two solves return the same bytes.
 *
 * DEPARTURES from the reference.  (1) Every step is exact up to cg_relative_tolerance where Theia runs ITERATIVE_SCHUR with Ceres'
 * inexact forcing sequence from 1000 views on and a direct Schur solver below.  (2) No inner iterations (Theia sets
 * use_inner_iterations = true).  (3) Points are inhomogeneous 3-vectors (as in gsfm_tracks_triangulate_refine); Theia optimises the
 * homogeneous 4-vector.  (4) p is formed with the matrix R where Theia rotates with AngleAxisRotatePoint.  (5) The gauge projection above.
 */
#ifndef GSFM_BA_H_
#define GSFM_BA_H_

#include <stdint.h>
#include "gsfm_rot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_BA_ABI_VERSION 1

typedef struct gsfm_ba_problem gsfm_ba_problem;

typedef struct {
  int32_t max_num_iterations;          /* 100 (Theia's BundleAdjustmentOptions) */
  int32_t jacobi_scaling;              /* 1 */
  double function_tolerance;           /* 1e-6 */
  double gradient_tolerance;           /* 1e-10 */
  double parameter_tolerance;          /* 1e-8 */
  double initial_trust_region_radius;  /* 1e4 */
  double max_trust_region_radius;      /* 1e12 (Theia's BundleAdjustmentOptions) */
  double min_trust_region_radius;      /* 1e-32 */
  double min_relative_decrease;        /* 1e-3 */
  double min_lm_diagonal;              /* 1e-6 */
  double max_lm_diagonal;              /* 1e32 */
  int32_t max_cg_iterations;           /* 2000 per LM step */
  int32_t cg_check_interval;           /* 8: PCG iterations between two read-backs of the residual */
  double cg_relative_tolerance;        /* 1e-12 */
  int32_t cg_stall_iterations;         /* 200: PCG also stops when its relative residual has not halved for this many iterations (0: never) */
  int32_t remove_gauge;                /* 1: project translation and scale out of every step (see above); 0: Ceres' plain step */
  int32_t verbose;                     /* 1: one line per LM iteration on stderr */
  int32_t reserved_;
} gsfm_ba_options;

typedef struct {
  int32_t termination;                 /* gsfm_rot_termination */
  int32_t num_iterations;
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_cg_iterations;           /* PCG iterations over all steps */
  int32_t num_pcg_stalled_steps;       /* steps whose PCG ended above cg_relative_tolerance */
  int32_t num_residual_sweeps;
  int32_t num_linearizations;
  int32_t nonfinite;                   /* 1 if a NaN / Inf cost was seen */
  int32_t reserved_;
  uint64_t num_observations_used;
  uint64_t num_active_cameras;
  uint64_t num_active_points;
  double initial_cost;
  double final_cost;
  double final_gradient_max_norm;
  double final_radius;
  double max_radius;
  double t_total_ms;
} gsfm_ba_summary;

int gsfm_ba_abi_version(void);
void gsfm_ba_options_default(gsfm_ba_options* options);

/* Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: a NULL required pointer, track_ptr[0] != 0, a track_ptr
 * that decreases, a camera index >= n_cams, 2^31 or more observations or nodes); without a device GSFM_ERR_NO_DEVICE.  A problem without
 * a used observation is valid: its solve changes nothing. */
gsfm_status gsfm_ba_problem_create(uint32_t n_cams, const double* rot_aa, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks,
                                   const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                   gsfm_ba_problem** out);
gsfm_status gsfm_ba_set_loss(gsfm_ba_problem* p, const gsfm_loss_node* program, int32_t n_nodes);
/* cam_pos_inout: n_cams x 3, point_inout: n_tracks x 3: start values in, estimates out (active nodes only are written).  options / summary may be NULL. */
gsfm_status gsfm_ba_solve(gsfm_ba_problem* p, double* cam_pos_inout, double* point_inout, const gsfm_ba_options* options, gsfm_ba_summary* summary);

/* ---- checks of the solve's own code (the tests compare them with a high-precision reference); every output may be NULL ---- */
/* r_out: n_obs x 2 (the plain residual), rho_out: n_obs (rho(s)); zeros for an unused observation */
gsfm_status gsfm_ba_residuals(gsfm_ba_problem* p, const double* cam_pos, const double* points, double* r_out, double* rho_out);
/* cost, gradient (n_cams x 3, n_tracks x 3) and the diagonal blocks B_k (n_cams x 9) and C_t (n_tracks x 9, row-major) at the point
 * given; zeros on inactive nodes.  The blocks H_e stay on the device for gsfm_ba_schur_matvec. */
gsfm_status gsfm_ba_linearize(gsfm_ba_problem* p, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                              double* diag_cam, double* diag_point);
/* y = Sc v (n_cams x 3) for the last gsfm_ba_linearize or gsfm_ba_step_check, with the Jacobi scale of that point (options->jacobi_scaling)
 * and D^2 at `radius`; the identity on inactive cameras. */
gsfm_status gsfm_ba_schur_matvec(gsfm_ba_problem* p, const double* v, double radius, const gsfm_ba_options* options, double* y);
/* One LM step's linear algebra at the point given, exactly as iteration 1 of gsfm_ba_solve computes it but at the given radius (the same
 * code), stopped before the accept / reject decision:
 *   rhs_out (n_cams x 3) the reduced right-hand side;  yc_out (n_cams x 3) the PCG solution;  yp_out (n_tracks x 3) the back-substituted
 *   points;  delta_cam_out / delta_point_out the step -S y after the gauge projection;
 *   scal_out[4]  model cost change, delta.g, delta^T L delta, PCG's final sqrt(r.M^-1 r / b.M^-1 b);   info_out[2]  PCG iterations, stalled (0 / 1) */
gsfm_status gsfm_ba_step_check(gsfm_ba_problem* p, const double* cam_pos, const double* points, double radius, const gsfm_ba_options* options,
                               double* rhs_out, double* yc_out, double* yp_out, double* delta_cam_out, double* delta_point_out, double* scal_out,
                               int32_t* info_out);
/* Mean device time in microseconds (HIP events, `reps` launches after a warm one) of the kernels of one linearisation and one Schur
 * product at the point given, damped at `radius`:  out_us[6] = point-side linearisation, camera-side linearisation, cost, point pass,
 * camera pass, preconditioner.  For tools/time_bundle_adjustment.py. */
gsfm_status gsfm_ba_time_kernels(gsfm_ba_problem* p, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us);
void gsfm_ba_problem_destroy(gsfm_ba_problem* p);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_BA_H_ */
