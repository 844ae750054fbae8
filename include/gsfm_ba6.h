/* gsfm_ba6.h -- C ABI of the full bundle adjustment on the GPU: camera orientations, camera positions and points (libgsfm_rot.so).
 *
 * Restates the solve of Theia's GlobalReconstructionEstimator::BundleAdjustment() (the body of the pipeline's
 * BundleAdjustmentAndRemoveOutlierPoints before SetOutlierTracksToUnestimated) with intrinsics_to_optimize = NONE: every camera's
 * orientation and position and every 3D point move together, the intrinsics are held.  gsfm_ba.h is the same problem with the
 * orientations held; this header follows it and states only what differs.
 *
 * Inputs are those of gsfm_ba_problem_create, except that rot_aa (n_cams x 3 angle-axis, world -> camera) is a start value and an unknown:
 * it is an argument of the solve, not of the problem.  Used observations, active, inactive and unestimated cameras and points are defined
 * as in gsfm_ba.h.  Inactive and unestimated nodes are no parameters: they pass through a solve bit for bit, orientations included.
 *
 * Definition.
 *   unknowns   per active camera the angle-axis vector w_k and the centre o_k, per active point X_t.  The orientation update is ADDITIVE
 *              in the angle-axis coordinates, w <- w + delta_w (Theia's BundleAdjuster sets no local parameterisation on the orientation),
 *              so Jacobi scaling and damping act on these coordinates.
 *   residual   p = R(w_k) (X_t - o_k),  r = (f p_x / p_z + u - x, f p_y / p_z + v - y),  s = |r|^2;  R = Ceres' AngleAxisToRotationMatrix.
 *   Jacobian   with P = (f / p_z) [[1, 0, -p_x / p_z], [0, 1, -p_y / p_z]]:  J_point = P R,  J_pos = -P R,  J_rot = -P [p]x J_l(w_k), where
 *              J_l(w) = I + (1 - cos t) / t^2 [w]x + (t - sin t) / t^3 [w]x^2 (t = |w|) is the left Jacobian of SO(3):
 *              d(R(w) v) / dw = -[R v]x J_l(w).  Ceres' Corrector is applied to the three 2 x 3 pieces as gsfm_ba.h applies it to J_point:
 *              J~ = sqrt(rho') (J - alpha / s r r^T J), r~ = sqrt(rho') / (1 - alpha) r.
 *   cost       1/2 sum rho(s) over the used observations.
 *   normal matrix   with the corrected camera Jacobian Jc_e = [J~_rot, -J~_point] (2 x 6) and Jp_e = J~_point: camera blocks
 *              B_k = sum_{e in k} Jc^T Jc (6 x 6, coordinates w then o), point blocks C_t = sum_{e in t} Jp^T Jp, off-diagonal blocks
 *              E_e = Jc^T Jp (6 x 3); gradient g_k = sum Jc^T r~, g_t = sum Jp^T r~.
 *   LM         the rules of gsfm_ba.h over 6 coordinates per camera: Jacobi scaling S = 1 / (1 + sqrt(diag)) from the start point, D^2 =
 *              clamp(S^2 diag, min_lm_diagonal, max_lm_diagonal) / radius, the step solves (S L S + D^2) y = S g, delta = -S y; model cost
 *              change -delta.g - |J~ delta|^2 / 2; invalid-step rule, acceptance, radius rule, function / gradient / parameter
 *              tolerances (norms over all active coordinates, the orientations' included).  gsfm_ba_options and gsfm_ba_summary are reused;
 *              the defaults are Theia's (100 iterations, radius 1e4 .. 1e12) and gsfm_ba6_options_default's PCG tolerance.
 *   linear solve    the points are eliminated: C~_t = S_t C_t S_t + D^2_t inverted per point by cofactors and Newton steps X <- X + X (I - C~ X)
 *              with the residual in double-double, the inverse kept as an unevaluated pair; the sums over a track's observations that it is
 *              applied to are accumulated as pairs too (far from the minimum a point's C~_t can be nearly singular, and in plain fp64 the
 *              reduced system inherits an error u cond(C~_t) through the cancellation in B~ - E~ C~^-1 E~^T).  With E~_e = S_k E_e S_t the reduced
 *              camera system  Sc y_c = b_c - E~ C~^-1 b_p,  Sc = B~ - E~ C~^-1 E~^T  has 6 x 6 diagonal blocks and is solved by preconditioned
 *              conjugate gradients from y_c = 0 until sqrt(r.M^-1 r / b.M^-1 b) <= cg_relative_tolerance (with the stall rule of
 *              gsfm_ba_options).  Sc is never formed and neither are the blocks: one product is a point pass, w_t = C~_t^-1 S_t sum_{e in t}
 *              Jp^T (Jc q_k(e)) with q = S v, then a camera pass, y_k = S_k sum_{e in k} Jc^T (Jc q_k - Jp S_t w_t(e)) + D^2_k v_k.  The
 *              preconditioner M is the 6 x 6 block diagonal of Sc (Ceres' SCHUR_JACOBI), S_k (sum_{e in k} Jc^T (I - Jp G_t Jp^T) Jc) S_k +
 *              D^2_k with G_t = S_t C~_t^-1 S_t, inverted per camera through its Cholesky factor (positive definite by the diagonal
 *              clamp).  The points follow by y_p = C~^-1 (b_p - E~^T y_c).
 *   gauge      J has seven null directions at every point: a common translation of all centres and points (3), scaling about the
 *              centroid of the active centres and points (1; orientations do not move), and a global rotation by phi (3):
 *              delta_X = phi x X, delta_o = phi x o, delta_w_k = -J_l(w_k)^-T phi.  Ceres and Theia fix nothing.  With remove_gauge = 1
 *              (default) every step loses its orthogonal projection onto the span of the seven: delta -= V c with (V^T V) c = V^T delta, V
 *              the seven directions on the active nodes in the order above.  The 28 + 7 dots are summed in a fixed order on the device,
 *              the 7 x 7 system is solved on the host by a Cholesky factorisation without pivoting; a direction whose pivot is not above
 *              1e-12 of its own squared norm (a degenerate scene) is left in the step.  J V = 0, so the model cost change is unchanged.
 *              remove_gauge = 0 is Ceres' plain step.  Compare results after removing a similarity transform.
 * The loss is one leaf or none, as for gsfm_ba_set_loss.
 *
 * Order of the sums (part of the definition).  As in gsfm_ba.h: sums over a track's observations run in lane groups of 4 / 16 / 64 lanes by
 * the track's CSR length (lane l adds the observations l, l + G, ... from 0, then the xor butterfly), sums over a camera's observations over
 * its used observations in ascending observation index (lane l of 64 adds the entries l, l + 64, ..., then the shuffle tree with offsets 32,
 * 16, ..., 1), global sums over 512 partials in a fixed order.  No atomics: two solves return the same bytes.
 *
 * DEPARTURES from the reference.  (1) Every step is exact up to cg_relative_tolerance where Theia runs ITERATIVE_SCHUR with Ceres' inexact
 * forcing sequence from 1000 views on and a direct Schur solver below.  (2) No inner iterations.  (3) Points are inhomogeneous 3-vectors;
 * Theia optimises the homogeneous 4-vector.  (4) p is formed with the matrix R where Theia rotates with AngleAxisRotatePoint, and the
 * orientation Jacobian is the closed form above where Ceres differentiates automatically.  (5) The gauge projection above.  (6) Intrinsics
 * are held (intrinsics_to_optimize = NONE, what the reference's flags_1dsfm.yaml sets; its flags.yaml sets FOCAL_LENGTH: gsfm_ba7.h).
 */
#ifndef GSFM_BA6_H_
#define GSFM_BA6_H_

#include <stdint.h>
#include "gsfm_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_BA6_ABI_VERSION 1

typedef struct gsfm_ba6_problem gsfm_ba6_problem;

int gsfm_ba6_abi_version(void);
/* gsfm_ba_options_default with cg_relative_tolerance = 1e-14 (what options == NULL means below).  With free orientations the reduced system is
 * worse conditioned than gsfm_ba.h's, and a PCG that stops right at 1e-12 leaves its truncation in the step: measured on a 12-camera scene
 * at radius 1e10, J~ delta was then twice as far from a high-precision step as 64 roundings of a direct solve allow, and within 0.02 of that
 * at 1e-14, for 1.0 to 1.6 times the PCG iterations. */
void gsfm_ba6_options_default(gsfm_ba_options* options);

/* Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: a NULL required pointer, track_ptr[0] != 0, a track_ptr
 * that decreases, a camera index >= n_cams, 2^31 or more observations or nodes; a node is an orientation, a centre or a point); without a
 * device GSFM_ERR_NO_DEVICE.  A problem without a used observation is valid: its solve changes nothing. */
gsfm_status gsfm_ba6_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                                    const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba6_problem** out);
gsfm_status gsfm_ba6_set_loss(gsfm_ba6_problem* p, const gsfm_loss_node* program, int32_t n_nodes);
/* rot_aa_inout, cam_pos_inout: n_cams x 3, point_inout: n_tracks x 3: start values in, estimates out (active nodes only are written).
 * options / summary may be NULL. */
gsfm_status gsfm_ba6_solve(gsfm_ba6_problem* p, double* rot_aa_inout, double* cam_pos_inout, double* point_inout, const gsfm_ba_options* options,
                           gsfm_ba_summary* summary);

/* ---- checks of the solve's own code (the tests compare them with a high-precision reference); every output may be NULL ---- */
/* r_out: n_obs x 2 (the plain residual), rho_out: n_obs (rho(s)); zeros for an unused observation */
gsfm_status gsfm_ba6_residuals(gsfm_ba6_problem* p, const double* rot_aa, const double* cam_pos, const double* points, double* r_out, double* rho_out);
/* cost, gradient (n_cams x 3 for the orientations and for the centres, n_tracks x 3) and the diagonal blocks B_k (n_cams x 36, row-major,
 * coordinates w then o) and C_t (n_tracks x 9) at the point given; zeros on inactive nodes.  The corrected Jacobians stay on the device
 * for gsfm_ba6_schur_matvec. */
gsfm_status gsfm_ba6_linearize(gsfm_ba6_problem* p, const double* rot_aa, const double* cam_pos, const double* points, double* cost, double* grad_rot,
                               double* grad_pos, double* grad_point, double* diag_cam, double* diag_point);
/* y = Sc v (n_cams x 6, per camera w then o) for the last gsfm_ba6_linearize or gsfm_ba6_step_check, with the Jacobi scale of that point
 * (options->jacobi_scaling) and D^2 at `radius`; the identity on inactive cameras. */
gsfm_status gsfm_ba6_schur_matvec(gsfm_ba6_problem* p, const double* v, double radius, const gsfm_ba_options* options, double* y);
/* One LM step's linear algebra at the point given, exactly as iteration 1 of gsfm_ba6_solve computes it but at the given radius (the same
 * code), stopped before the accept / reject decision:
 *   rhs_out, yc_out (n_cams x 6, per camera w then o) the reduced right-hand side and the PCG solution;  yp_out (n_tracks x 3) the
 *   back-substituted points;  delta_rot_out / delta_pos_out / delta_point_out the step -S y after the gauge projection;  jdelta_out
 *   (n_obs x 2) J~ delta per observation (zeros for an unused one);
 *   scal_out[4]  model cost change, delta.g, |J~ delta|^2, PCG's final sqrt(r.M^-1 r / b.M^-1 b);   info_out[2]  PCG iterations, stalled (0 / 1) */
gsfm_status gsfm_ba6_step_check(gsfm_ba6_problem* p, const double* rot_aa, const double* cam_pos, const double* points, double radius,
                                const gsfm_ba_options* options, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out,
                                double* delta_pos_out, double* delta_point_out, double* jdelta_out, double* scal_out, int32_t* info_out);
/* Mean device time in microseconds (HIP events, `reps` launches after a warm one) of the kernels of one linearisation and one Schur
 * product at the point given, damped at `radius`:  out_us[8] = camera records, point-side linearisation, camera-side linearisation, cost,
 * point pass, camera pass, preconditioner, quadratic form.  For tools/time_full_bundle_adjustment.py. */
gsfm_status gsfm_ba6_time_kernels(gsfm_ba6_problem* p, const double* rot_aa, const double* cam_pos, const double* points, double radius, int32_t reps,
                                  double* out_us);
void gsfm_ba6_problem_destroy(gsfm_ba6_problem* p);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_BA6_H_ */
