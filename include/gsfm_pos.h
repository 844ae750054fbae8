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


/* The 1DSfM outlier filter of relative translations (Wilson and Snavely), Theia's FilterViewPairsFromRelativeTranslation
 * (filter_view_pairs_from_relative_translation.cc), on flat arrays and on the device.  The reference's result depends on the iteration
 * order of its hash maps and on libstdc++'s normal_distribution; this entry keeps every rule of the reference that decides something
 * and fixes what the reference leaves to chance, so that two calls return the same bytes:
 *   1. world directions  d_e = R(aa_i)^T t_e (t_e = position_2, used as given, not normalised; the position problem's routine).
 *   2. mean = sum d_e / E, var = sum (d_e - mean)^2 / (E - 1) per component (0 for E = 1), reduced in a fixed order.
 *   3. axes == NULL: axis_k = normalise(mean + var o z_k), z_k standard normal.  The reference hands the VARIANCE to a parameter named
 *      std_dev; that is kept.  The normals come from the library's own generator (splitmix64 + Box-Muller, host code) seeded with
 *      `seed` (the reference's pipeline seeds with 1): these are NOT the reference's axes.  axes != NULL: n_axes x 3, used as given.
 *   4. projections  p_ek = d_e . axis_k  = fma(d2, a2, fma(d1, a1, d0 a0)).
 *   5. under projection k edge e is the arc i -> j if p_ek > 0, else j -> i (p == 0: a reversed arc of weight 0), with the INTEGER
 *      weight q_ek = floor(|p_ek| 2^32 + 0.5).  Integer weights are the one deliberate departure in the arithmetic: their sums are exact,
 *      so a camera's in- and out-weight do not depend on the order in which its neighbours are removed.  Input whose per-camera sums
 *      could reach 2^62 is rejected (with |t| <= 1 and unit axes: a camera of about 2^30 edges).
 *   6. ordering.  Nodes: the cameras that appear in an edge.  Per live node qin, qout (sums over arcs from / to live nodes) and indeg
 *      (live incoming arcs, zero-weight arcs included).  Until no node is live: if any live node has indeg == 0, ALL such nodes are
 *      removed (they are pairwise non-adjacent, and removing one never stops another from being a source, so every order of removing
 *      them leaves each edge on the same side -- the reference removes them one at a time in hash order); otherwise the one live node
 *      with the largest score double(qout + 2^32) / double(qin + 2^32) (the reference's (out + 1) / (in + 1)) is removed, the smallest
 *      camera index among equal scores (the reference: whichever its hash map meets first).  A removed node gets the number of its pass.
 *   7. edge e is inconsistent under projection k when its arc's tail was removed in a later pass than its head;
 *      bad_e = sum_k [inconsistent] |p_ek| in fp64, k ascending.
 *   8. keep_e = !(bad_e > tolerance * n_axes).
 * rot_aa is read for the first camera of every edge only.  A repeated pair is a parallel arc.  Outputs: bad_weight_out, keep_out (n_edges
 * each, required), n_kept; optional (NULL: not returned) stats_out[6] (mean, var), axes_out (n_axes x 3: the axes used), proj_out
 * (n_edges x n_axes, row per edge; computed only on request -- the ordering recomputes projections from the directions and never stores
 * them), num_passes_out / num_picks_out (n_axes each: passes of step 6 and how many of them picked by score), kernel_ms (device time of
 * all kernels).  Device memory O(n_edges + n_axes n_cams).  Arguments are checked on the host before any device call
 * (GSFM_ERR_INVALID_ARG); without a device GSFM_ERR_NO_DEVICE: there is no host fallback.  No edges: GSFM_OK, n_kept = 0. */
gsfm_status gsfm_pos_filter_relative_translations(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                                  const double* rot_aa, int32_t n_axes, const double* axes, uint64_t seed, double tolerance,
                                                  double* bad_weight_out, uint8_t* keep_out, uint64_t* n_kept, double* stats_out, double* axes_out,
                                                  double* proj_out, uint32_t* num_passes_out, uint32_t* num_picks_out, double* kernel_ms);

/* Relative translations refined with known rotations: Theia's RefineRelativeTranslationsWithKnownRotations (reconstruction_estimator_utils.cc)
 * -> OptimizeRelativePositionWithKnownRotation, one small problem per view pair over the pair's matched features, on flat arrays and on
 * the device.  The reference's random start is overwritten before it is read, so the result is deterministic.  For edge e = (i, j) with
 * matches m = match_ptr[e] .. match_ptr[e + 1] - 1 (n of them) and intrinsics f1 u1 v1 f2 u2 v2 (those of gsfm_cov_estimate):
 *   1. features     f1_m = ((x1 - u1) / f1, (y1 - v1) / f1, 1), f2_m likewise from (x2, y2) and the second camera's intrinsics.
 *   2. constraints  a_m = R1 ((R2^T f2_m) x (R1^T f1_m)), R1 = R(aa_i), R2 = R(aa_j) (Ceres' AngleAxisToRotationMatrix): three components,
 *      in the frame of camera i like position_2.
 *   3. IRLS         w_m = 1, cost = 0, inner = 0; at most 100 iterations, stopping once inner reaches 10.  One iteration:
 *        w_m <- max(w_m, 1e-7);  L = sum_m a_m a_m^T / w_m;
 *        t = unit eigenvector of the smallest eigenvalue of L (Theia: the last left singular vector; its sign is free and nothing
 *            here depends on it).  L is divided by its trace first; cyclic Jacobi in fp64 over the pairs (0,1), (0,2), (1,2), a pair
 *            rotated when |L_pq| > 2^-54 sqrt(|L_pp L_qq|), until a sweep rotates nothing (16 sweeps at most);
 *        w_m <- |t . a_m|;  new_cost = sum_m w_m (the unfloored weights);
 *        delta = max(|cost - new_cost|, 1 - t.t);  inner <- inner + 1 if delta <= 1e-5, else 0;  cost <- new_cost.
 *   4. sign         with Rrel = R2 R1^T, d1 = f1_m, d2 = Rrel^T f2_m a match lies in front of both cameras when
 *        d2.d2 d1.t - d1.d2 d2.t > 0  and  d1.d2 d1.t - d1.d1 d2.t > 0;   t is negated unless more than n / 2 (integer division) do.
 *      (When neither t nor -t has such a majority -- a pair whose fit went wrong -- the result is the negated eigenvector, whose sign
 *      is the eigen-solver's choice; the reference has the same gap.  The Jacobi solve is deterministic, so the bytes still repeat.)
 * The sums run in a fixed order (lane l of a 64-lane wavefront adds matches l, l + 64, ..., then an xor-butterfly), and an edge's result
 * depends on that edge's data alone: two calls return the same bytes, and reordering the edges reorders the outputs bit for bit.
 * rel_t_out (n_edges x 3): the unit vector t, to be stored as the pair's position_2.  status_out per edge:
 *   0  refined;
 *   1  skipped: fewer than 2 matches; rel_t_out = rel_t_in, 0 iterations, cost 0;
 *   2  a non-finite result (the trace of L is not a positive finite number in some iteration -- all-zero constraints, non-finite
 *      input -- or t or the cost is not finite at the end); rel_t_out = rel_t_in, cost 0, iters_out = the iterations completed.
 * iters_out (iterations of step 3), cost_out (the final cost of step 3), kernel_ms (device time of the kernel) may be NULL.  matches:
 * match_ptr[n_edges] rows of x1 y1 x2 y2 in pixels (may be NULL when there are none).  Device memory 56 B per match + O(n_edges + n_cams).
 * Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: a NULL required pointer, a camera index >= n_cams, a
 * match_ptr that decreases); without a device GSFM_ERR_NO_DEVICE: there is no host fallback.  No edges: GSFM_OK. */
gsfm_status gsfm_pos_refine_relative_translations(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j,
                                                  const uint64_t* match_ptr, const double* matches, const double* intrinsics,
                                                  const double* rot_aa, const double* rel_t_in, double* rel_t_out, int32_t* status_out,
                                                  int32_t* iters_out, double* cost_out, double* kernel_ms);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_POS_H_ */
