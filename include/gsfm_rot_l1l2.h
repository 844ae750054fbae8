/* gsfm_rot_l1l2.h -- C ABI of the robust L1 + IRLS rotation estimator on the GPU (libgsfm_rot.so).
 *
 * Restates Theia's RobustRotationEstimator (sfm/global_pose_estimation/robust_rotation_estimator.{h,cc}, math/l1_solver.h), the method of
 * Chatterjee and Govindu, "Efficient and Robust Large-Scale Rotation Averaging" (ICCV 2013): Theia's ROBUST_L1L2.
 *
 * Input and parameters.  n_cams cameras, E edges (i, j, rel_aa), start rotations rot_aa (n_cams x 3, angle-axis) and fixed_cam.  Cameras
 * that appear in no edge are not parameters: they pass through untouched.  N is the number of cameras that appear in an edge.  The unknown
 * step x has 3 (N - 1) entries; the fixed camera has no column.
 *
 * Residual.  b_e = Log(R_j^T R_ij R_i), with R = Ceres' AngleAxisToRotationMatrix and Log = Ceres' RotationMatrixToAngleAxis, which goes
 * through the quaternion: the angle lies in (-pi, pi].  The library keeps the rotations as unit quaternions during a call; the reference's
 * angle-axis round trip between the two products is not replayed.
 *
 * Matrix.  (A x)_e = x_j - x_i, the fixed camera's term left out: A = B (x) I3 with B the signed edge-camera incidence matrix, so
 * A^T A = L (x) I3 and A^T W A = L_w (x) I3 with L a scalar graph Laplacian, the fixed camera grounded.
 *
 * L1 stage (SolveL1Regression).  inner = admm_initial_iterations (5), x = 0.  At most max_num_l1_iterations (5) outer iterations; each
 * runs ADMM on min |A x - b|_1 with rho = admm_rho (1), alpha = admm_alpha (1), from z = u = 0, for at most `inner` iterations:
 *     x     = (A^T A)^-1 A^T (b + z - u)
 *     h     = alpha A x + (1 - alpha) (z + b)                  (h = A x at alpha = 1)
 *     z_old = z;   z = shrink(h - b + u, 1 / rho);   u += h - z - b            shrink(v, k) = max(0, v - k) - max(0, -v - k)
 *     stop when  |A x - z - b| < sqrt(3 E) abs + rel max(|A x|, |z|, |b|)
 *          and   |rho A^T (z - z_old)| < sqrt(3 (N - 1)) abs + rel |rho A^T u|
 *   abs = admm_absolute_tolerance (1e-4), rel = admm_relative_tolerance (1e-2), 2-norms, u the updated one.  Then R_k <- R_k Exp(x_k) for
 *   every free camera (MultiplyRotations(rotation, change)), b is recomputed, avg = mean over the free cameras of |x_k|.  The stage stops
 *   when avg <= l1_step_convergence_threshold (1e-3); otherwise inner *= 2.
 *
 * IRLS stage (SolveIRLS).  At most max_num_irls_iterations (100) iterations: w_e = sigma / (|b_e|^2 + sigma^2)^2 with
 * sigma = irls_loss_parameter_sigma (5 degrees, in radians); x = (A^T W A)^-1 A^T W b; the rotations are updated, b is recomputed; the
 * stage stops when avg < irls_step_convergence_threshold (1e-3, strict).
 *
 * What the reference leaves open is fixed here, so that a call is a function of its arguments:
 *   - fixed_cam names the camera held constant (the reference: whichever view its hash map lists first).
 *   - Edges are used as listed: i > j is allowed, and the same pair may appear several times (AddRelativeRotationConstraint allows it).
 *   - Refused on the host before anything is launched (GSFM_ERR_INVALID_ARG, the message in gsfm_last_error): edge_i == edge_j; an index
 *     >= n_cams; a non-finite rel_aa, or a non-finite start rotation of a camera that has an edge; a fixed_cam without an edge; a camera
 *     with an edge that is not connected to fixed_cam (the reference's Cholesky fails there; a union-find at entry finds it).
 *   - The linear solves are one Jacobi-preconditioned PCG on the 3 (N - 1) system, the preconditioner the (weighted) degree, each held
 *     to cg_relative_tolerance on sqrt(r.M^-1 r / b.M^-1 b).  A right-hand side of zero gives x = 0.  A solve that stalls or reaches
 *     max_cg_iterations is counted (num_pcg_stalled_solves) and used all the same.
 *   - Every sum runs in a fixed order and nothing uses floating-point atomics: two calls on the same input return the same bytes.
 *   - A camera whose every step was exactly zero keeps the bytes of its start rotation.
 * Without a device GSFM_ERR_NO_DEVICE: there is no host fallback.
 */
#ifndef GSFM_ROT_L1L2_H_
#define GSFM_ROT_L1L2_H_

#include <stdint.h>
#include "gsfm_rot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_ROT_L1L2_ABI_VERSION 1
#define GSFM_ROT_L1L2_MAX_L1 8           /* per-outer-iteration records kept in the summary */

typedef struct {
  int32_t max_num_l1_iterations;           /* 5     (Theia RobustRotationEstimator::Options) */
  int32_t max_num_irls_iterations;         /* 100   */
  double l1_step_convergence_threshold;    /* 1e-3  */
  double irls_step_convergence_threshold;  /* 1e-3  */
  double irls_loss_parameter_sigma;        /* 5 degrees in radians */
  int32_t admm_initial_iterations;         /* 5: ADMM iterations of the first outer iteration, doubled after each (SolveL1Regression) */
  int32_t max_cg_iterations;               /* 2000 per linear solve */
  double admm_rho;                         /* 1     (Theia L1Solver::Options) */
  double admm_alpha;                       /* 1     */
  double admm_absolute_tolerance;          /* 1e-4  */
  double admm_relative_tolerance;          /* 1e-2  */
  double cg_relative_tolerance;            /* 1e-14: PCG stops when sqrt(r.M^-1 r / b.M^-1 b) <= this (the table) */
  int32_t cg_check_interval;               /* 4: PCG iterations between two looks at the residual */
  int32_t cg_stall_iterations;             /* 200: PCG gives up when r.M^-1 r has not quartered for so many iterations (0: never) */
  int32_t verbose;                         /* 1: one line per ADMM / outer / IRLS iteration on stderr */
  int32_t reserved_;
} gsfm_rot_l1l2_options;

typedef struct {
  int32_t num_l1_iterations;                          /* outer iterations of the L1 stage run */
  int32_t num_admm_iterations[GSFM_ROT_L1L2_MAX_L1];  /* ADMM iterations of each (the first GSFM_ROT_L1L2_MAX_L1 of them) */
  int32_t num_irls_iterations;
  int32_t l1_converged;                               /* 1: the stage ended on its threshold, 0: on its cap */
  int32_t irls_converged;
  int32_t num_cg_iterations;                          /* PCG iterations over all solves */
  int32_t num_linear_solves;
  int32_t num_pcg_stalled_solves;                     /* solves that ended above cg_relative_tolerance (stall rule or cap) */
  int32_t nonfinite;                                  /* 1 if a norm or a step size read back was NaN / Inf (the call stops there) */
  uint64_t num_edges_used;
  double l1_step[GSFM_ROT_L1L2_MAX_L1];               /* avg after each outer iteration */
  double last_irls_step;                              /* avg of the last IRLS iteration */
  double worst_accepted_cg_residual;                  /* largest final sqrt(r.M^-1 r / b.M^-1 b) over all solves */
  double t_total_ms;
  double kernel_ms;                                   /* device time from the first kernel to the last */
} gsfm_rot_l1l2_summary;

int gsfm_rot_l1l2_abi_version(void);
void gsfm_rot_l1l2_options_default(gsfm_rot_l1l2_options* options);

/* edge_i, edge_j: n_edges camera indices; rel_aa: n_edges x 3; rot_aa_inout: n_cams x 3 start rotations in, estimates out (written only
 * on GSFM_OK); options / summary may be NULL.  One flat call: a private stream, one slab, nothing kept between calls. */
gsfm_status gsfm_rot_l1l2_solve(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                                double* rot_aa_inout, int32_t fixed_cam, const gsfm_rot_l1l2_options* options, gsfm_rot_l1l2_summary* summary);

/* Two testing aids: checks of the solve's own code (the tests compare them with a high-precision reference and a dense solution).
 *
 * gsfm_rot_l1l2_residuals: b (n_edges x 3) at the rotations rot_aa, by the solve's edge sweep; sq_out (n_edges, |b_e|^2) and weight_out
 * (n_edges, the IRLS weight at options->irls_loss_parameter_sigma) may be NULL.  Only the edges' indices and values are checked.
 *
 * gsfm_rot_l1l2_laplacian_solve: the solve's own structure, product and PCG on a given right-hand side: x = L_w^-1 rhs on the free
 * cameras.  weights: n_edges positive weights, or NULL for the unweighted form (which reads no weight array).  rhs: n_cams x 3, read on
 * the free cameras; x_out: n_cams x 3, zero elsewhere.  info_out[6] (may be NULL): PCG iterations, 1 if stalled or capped, the final
 * sqrt(r.M^-1 r / b.M^-1 b), the device time of the solve in ms, the device time of one product in ms (the mean of 20 launched back
 * to back after the solve, which a call with info_out pays for) and the bytes one product streams, computed from the shapes.  The graph is checked as gsfm_rot_l1l2_solve checks it. */
gsfm_status gsfm_rot_l1l2_residuals(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                                    const double* rot_aa, const gsfm_rot_l1l2_options* options, double* b_out, double* sq_out, double* weight_out);
gsfm_status gsfm_rot_l1l2_laplacian_solve(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* weights,
                                          int32_t fixed_cam, const double* rhs, const gsfm_rot_l1l2_options* options, double* x_out, double* info_out);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_ROT_L1L2_H_ */
