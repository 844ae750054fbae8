/* gsfm_pos.h -- C ABI of camera-position estimation on the GPU (libgsfm_rot.so).
 *
 * Restates the reference's GSfMNonlinearPositionEstimator::EstimatePositions (src/GSfM_nonlinear_position_estimator.cpp) with
 * camera-to-camera BASELINE constraints and no point constraints:
 *   one residual per view-graph edge (i, j):   r = (c_j - c_i) / n - R(aa_i)^T t_ij,   n = |c_j - c_i|, n := 1 below 1e-12
 *   (Theia's PairwiseTranslationError; R = Ceres' AngleAxisToRotationMatrix; t_ij = TwoViewInfo::position_2, used as given),
 * weight 1, robustified by the loss through Ceres' Corrector, minimised by Levenberg-Marquardt with Ceres 1.14's trust-region rules.
 * One camera is held constant (the reference fixes positions->begin() at zero).  The loss descriptors are those of gsfm_rot.h; a new
 * problem has Ceres' NULL loss (the estimator layer sets the reference's default, HuberLoss(0.1)).
 *
 * Linear solver.  Every LM step is EXACT up to the solver's precision: a dense Cholesky of the damped, Jacobi-scaled normal matrix up to
 * dense_max_cams cameras (the reference's SPARSE_NORMAL_CHOLESKY regime, <= 1000 cameras), block-Jacobi PCG held to cg_relative_tolerance
 * beyond.  The reference switches to CGNR with Ceres' default forcing sequence above 1000 cameras, i.e. to INEXACT steps; this library
 * keeps exact steps everywhere and makes its parity claims at exact steps (as gsfm_rot.h does for rotations, see cg_relative_tolerance).
 *
 * Scale gauge.  The cost is invariant under c -> c_0 + lambda (c - c_0) about the fixed camera c_0, so v = c - c_0 is a null vector of
 * J^T J and only the LM damping makes the step system definite; its condition number grows with the trust-region radius.  With
 * remove_scale_gauge = 1 (default) each step's component along v is removed (delta -= (delta.v / v.v) v) before it is evaluated -- a
 * departure from Ceres, which leaves that component to the damping: J v = 0, so the model cost change is unchanged, and the step no
 * longer depends on how a solver resolves a direction the cost cannot see.  Compare positions after removing translation and scale.
 */
#ifndef GSFM_POS_H_
#define GSFM_POS_H_

#include <stdint.h>
#include "gsfm_rot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_POS_ABI_VERSION 2

typedef struct gsfm_pos_problem gsfm_pos_problem;

typedef struct {
  int32_t max_num_iterations;          /* 400 (Theia NonlinearPositionEstimator::Options) */
  int32_t jacobi_scaling;              /* 1: Ceres' Jacobi scaling, computed once from the Jacobian at the start point */
  double function_tolerance;           /* 1e-6  Ceres 1.14 defaults from here on */
  double gradient_tolerance;           /* 1e-10 */
  double parameter_tolerance;          /* 1e-8  */
  double initial_trust_region_radius;  /* 1e4   */
  double max_trust_region_radius;      /* 1e16  */
  double min_trust_region_radius;      /* 1e-32 */
  double min_relative_decrease;        /* 1e-3  */
  double min_lm_diagonal;              /* 1e-6  */
  double max_lm_diagonal;              /* 1e32  */
  int32_t dense_max_cams;              /* 1000: exact steps by dense Cholesky up to this many cameras (and 5333 at most), PCG beyond */
  int32_t max_cg_iterations;           /* 2000 per LM step */
  double cg_relative_tolerance;        /* 1e-12: PCG stops when sqrt(r.M^-1 r / b.M^-1 b) <= this */
  int32_t cg_check_interval;           /* 8: PCG iterations between two read-backs of the residual */
  int32_t cg_stall_iterations;         /* 200: PCG also stops when its relative residual has not halved for this many iterations
                                          (0: never); such a step is counted in num_pcg_stalled_steps and evaluated all the same */
  int32_t remove_scale_gauge;          /* 1: project the scale-gauge direction out of every step (see above); 0: Ceres' plain step */
  int32_t verbose;                     /* 1: one line per LM iteration on stderr */
} gsfm_pos_options;

typedef struct {
  int32_t termination;                 /* gsfm_rot_termination */
  int32_t num_iterations;              /* LM iterations */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_cg_iterations;           /* PCG iterations over all steps */
  int32_t num_dense_solves;            /* steps solved by the dense Cholesky */
  int32_t num_pcg_stalled_steps;       /* PCG steps that ended above cg_relative_tolerance (stall rule or max_cg_iterations) */
  int32_t num_residual_sweeps;         /* cost evaluations (start point and trial points) */
  int32_t num_linearizations;
  int32_t nonfinite;                   /* 1 if a NaN / Inf cost was seen */
  uint64_t num_edges_used;
  double initial_cost;
  double final_cost;
  double final_gradient_max_norm;
  double final_radius;
  double max_radius;                   /* largest trust-region radius of the run */
  double t_total_ms;
} gsfm_pos_summary;

int gsfm_pos_abi_version(void);
void gsfm_pos_options_default(gsfm_pos_options* options);

/* edge_i, edge_j: n_edges camera indices < n_cams, edge_i != edge_j; rel_t: n_edges x 3 (position_2 of each view pair, in the frame of
 * camera i); rot_aa: n_cams x 3 angle-axis orientations (read for the cameras that appear in an edge).  Cameras without an edge are not
 * parameters: their positions pass through a solve untouched.  The edges' world directions are computed on the device here. */
gsfm_status gsfm_pos_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                    const double* rot_aa, gsfm_pos_problem** out);
gsfm_status gsfm_pos_set_loss(gsfm_pos_problem* p, const gsfm_loss_node* program, int32_t n_nodes);   /* n_nodes = 0: Ceres' NULL loss */
gsfm_status gsfm_pos_set_loss_callback(gsfm_pos_problem* p, gsfm_loss_callback fn, void* user);
/* pos_inout: n_cams x 3 start positions in, estimates out.  fixed_cam: the camera held constant (must appear in an edge), or -1 for none.
 * options / summary may be NULL. */
gsfm_status gsfm_pos_solve(gsfm_pos_problem* p, double* pos_inout, int32_t fixed_cam, const gsfm_pos_options* options, gsfm_pos_summary* summary);
/* residuals at pos: r_out n_edges x 3, rho_out n_edges (rho(|r|^2) of the loss; either may be NULL) */
gsfm_status gsfm_pos_residuals(gsfm_pos_problem* p, const double* pos, double* r_out, double* rho_out);
/* Checks of the solve's own code (the tests compare them with a high-precision reference).
 *
 * gsfm_pos_linearize: the cost and the linearisation at pos with every present camera active, as a solve evaluates them (callback loss
 * included): gradient g = J~^T r~ (n_cams x 3), the diagonal blocks D_k = sum_e H_e of J~^T J~ (n_cams x 9, row-major) and the cost
 * (each may be NULL).  The per-entry blocks H_e stay on the device for gsfm_pos_normal_matvec.
 * A NaN gradient entry is not counted in a solve's final_gradient_max_norm (fmax drops it, as the oracle's std::fmax does).          */
gsfm_status gsfm_pos_linearize(gsfm_pos_problem* p, const double* pos, double* gradient, double* diag_blocks, double* cost);
/* y = L v with L = J~^T J~ of the last gsfm_pos_linearize or gsfm_pos_step_check: y_k = sum_e H_e (v_k - v_m) on the active rows of that
 * call and 0 on inactive rows.  v is used as given, on inactive cameras too (a neighbour's v_m enters y_k whether or not m is active). */
gsfm_status gsfm_pos_normal_matvec(gsfm_pos_problem* p, const double* v, double* y);
/* One LM step's linear algebra at pos, exactly as iteration 1 of gsfm_pos_solve(pos, fixed_cam, o) computes it but at the given radius
 * (the same code): the linearisation, the Jacobi scale S of pos, D^2 = clamp(S^2 diag(L), min_lm_diagonal, max_lm_diagonal) / radius,
 * the damped system K y = b with K = S L S + D^2 and b = S g (the identity and 0 on inactive rows), solved by the dense Cholesky (up to
 * o->dense_max_cams cameras) or PCG, the step delta = -S y with its scale-gauge part removed, and the model cost change.  No accept or
 * reject decision; the solve's state is not an input.  o may be NULL (defaults).  Outputs (each may be NULL):
 *   K_out      (3 n_cams)^2 row-major, full symmetric: K as assembled for the dense Cholesky (written only when the dense path assembled it)
 *   b_out, y_out, delta_out   3 n_cams each
 *   scal_out[4]   model cost change -delta.g - delta^T L delta / 2, delta.g, delta^T L delta, PCG's final sqrt(rz / rz0) (0 on the dense path)
 *   info_out[3]   path (0 dense, 1 PCG), the Cholesky's info (-1: not run, > 0: a non-positive pivot, then PCG), PCG iterations       */
gsfm_status gsfm_pos_step_check(gsfm_pos_problem* p, const double* pos, int32_t fixed_cam, double radius, const gsfm_pos_options* o, double* K_out,
                                double* b_out, double* y_out, double* delta_out, double* scal_out, int32_t* info_out);
void gsfm_pos_problem_destroy(gsfm_pos_problem* p);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_POS_H_ */
