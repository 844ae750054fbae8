// Device kernel of the track triangulation with the per-track refinement (include/gsfm_tracks.h, gsfm_tracks_triangulate_refine): Theia's
// TrackEstimator::EstimateTrack with bundle_adjustment = true -- midpoint, BundleAdjustTrack (Levenberg-Marquardt on the point alone, the
// cameras held), reprojection gate -- under the definition of that header.
//
//   k_tri_refine_tracks<G>  the lane group, the lane classes and the launch order of k_tri_tracks<G> (triangulate_kernels.hpp).  One launch
//                           does front (tri_front: rays, angle, midpoint), LM and gate (tri_gate): the point, the ten sums of a pass and
//                           every scalar of the trust region stay in registers from the midpoint to the stores.
//     pass      lane l of the group takes observations l, l + G, ... of the track at a point X: reprojection residual, loss, Ceres'
//               corrector, the 2 x 3 Jacobian; six sums of J^T J, three of g = J^T f, the cost; ten xor butterflies give every lane the
//               same sums.  The camera record (128 B) and the pixel (16 B) are gathered again in every pass: they are L2 hits after the
//               front, and holding them would cost 34 VGPRs per observation a lane owns.
//     iteration every lane solves the damped 3 x 3 system by Cholesky and takes every scalar decision on the same values, so the lanes of
//               a group agree without a vote.  ONE pass per iteration: the trial point's cost and its linearisation are formed together,
//               an accepted trial is the next iterate, a rejected one is dropped.
// Groups of a wavefront finish at different iterations: a finished group runs along masked (its pass is evaluated at its final point and
// thrown away) until the wavefront's last group is done -- the butterflies need every lane.  The loop is bounded by max_num_iterations
// (the host clamps it to 0 .. GSFM_TRR_MAX_ITERATIONS): no atomics, nothing waits for another work-group, no host round trip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "triangulate_kernels.hpp"
#include "loss_dev.hpp"
#include "reproj_dev.hpp"

namespace gsfm {

#define GSFM_TRR_MAX_ITERATIONS 1000
#define GSFM_TRR_MAX_INVALID_STEPS 5

struct TriRefineArgs {
  TriArgs tri;
  DevLossNode leaf;              // the one simple leaf of the loss (TRIVIAL for the NULL loss)
  int32_t max_num_iterations;    // 0 .. GSFM_TRR_MAX_ITERATIONS
  double function_tolerance, gradient_tolerance, parameter_tolerance, min_relative_decrease;
  double initial_radius, max_radius, min_radius;
  int32_t* iterations;
  int32_t* termination;          // gsfm_rot_termination, -1 for a track that is not refined
  double* initial_cost;
  double* final_cost;
};

// One pass at the point X: S = J^T J (xx xy xz yy yz zz), g (x y z), cost -- the same values in every lane of the group.
template <int G>
__device__ __forceinline__ void trr_pass(const TriArgs& a, const DevLossNode& leaf, const TriTrack& tk, int l, const double* X, double* S) {
  double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const double* cam = a.cams + (uint64_t)GSFM_TRI_CAM_DOUBLES * a.obs_cam[tk.ob + k];
    if (cam[15] == 0.0) continue;
    const double2 xy = a.obs_xy[tk.ob + k];
    const double v0 = X[0] - cam[9], v1 = X[1] - cam[10], v2 = X[2] - cam[11];
    double J0[3], J1[3], r0, r1, rho0;
    reproj_corrected(cam, xy, v0, v1, v2, leaf, J0, J1, r0, r1, rho0);   // (reproj_dev.hpp: shared with the bundle adjustment)
    s[0] += J0[0] * J0[0] + J1[0] * J1[0]; s[1] += J0[0] * J0[1] + J1[0] * J1[1]; s[2] += J0[0] * J0[2] + J1[0] * J1[2];
    s[3] += J0[1] * J0[1] + J1[1] * J1[1]; s[4] += J0[1] * J0[2] + J1[1] * J1[2]; s[5] += J0[2] * J0[2] + J1[2] * J1[2];
    s[6] += J0[0] * r0 + J1[0] * r1; s[7] += J0[1] * r0 + J1[1] * r1; s[8] += J0[2] * r0 + J1[2] * r1;
    s[9] += 0.5 * rho0;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) S[k] = tri_group_allsum<G>(s[k]);
}

__device__ __forceinline__ double trr_gmax(const double* S) { return fmax(fabs(S[6]), fmax(fabs(S[7]), fabs(S[8]))); }

template <int G>
__global__ void __launch_bounds__(G == 64 ? 64 : GSFM_TRI_BLOCK) k_tri_refine_tracks(TriRefineArgs r) {
  constexpr int BLOCK = G == 64 ? 64 : GSFM_TRI_BLOCK;
  constexpr int GROUPS = BLOCK / G;
  constexpr int CAP = G == 4 ? GSFM_TRI_LEN_G4 : GSFM_TRI_LEN_G16;
  __shared__ double lds_rays[G == 64 ? 1 : 3 * GROUPS * CAP];
  const TriArgs& a = r.tri;
  const int group = threadIdx.x / G, l = threadIdx.x % G, lane_in_wave = threadIdx.x & 63;
  const TriTrack tk = tri_track<G>(a, lds_rays, group);
  double X[3], mean = 0.0;
  int n;
  int status = tri_front<G>(a, tk, l, lane_in_wave, X, n);

  // ---- the refinement: Ceres 1.14's TrustRegionMinimizer with the Levenberg-Marquardt strategy on the three coordinates ----
  double S[10];
  trr_pass<G>(a, r.leaf, tk, l, X, S);
  const double initial_cost = S[9];
  double x_cost = S[9], gmax = trr_gmax(S), radius = r.initial_radius, decrease_factor = 2.0;
  const double sc[3] = {1.0 / (1.0 + sqrt(S[0])), 1.0 / (1.0 + sqrt(S[3])), 1.0 / (1.0 + sqrt(S[5]))};   // Jacobi scaling, taken at the midpoint
  int term = -1, it = 0, num_invalid = 0;
  bool last_successful = false;
  if (status == 0) {
    if (!isfinite(x_cost)) term = GSFM_TERM_FAILURE;
    else if (gmax <= r.gradient_tolerance) term = GSFM_TERM_GRADIENT_TOLERANCE;
    else if (r.max_num_iterations <= 0) term = GSFM_TERM_NO_CONVERGENCE;
  }
  bool done = status != 0 || term >= 0;
  for (int step = 0; step < r.max_num_iterations; ++step) {
    if (__ballot(!done) == 0ull) break;                  // the wavefront's last group is done
    // (J_s^T J_s + D^2 / radius) d_s = -g_s in the scaled space, J_s = J diag(sc)
    const double a00 = S[0] * sc[0] * sc[0], a01 = S[1] * sc[0] * sc[1], a02 = S[2] * sc[0] * sc[2];
    const double a11 = S[3] * sc[1] * sc[1], a12 = S[4] * sc[1] * sc[2], a22 = S[5] * sc[2] * sc[2];
    const double g0 = S[6] * sc[0], g1 = S[7] * sc[1], g2 = S[8] * sc[2];
    const double p0 = a00 + fmin(fmax(a00, 1e-6), 1e32) / radius;
    const double l00 = sqrt(p0), l10 = a01 / l00, l20 = a02 / l00;
    const double p1 = a11 + fmin(fmax(a11, 1e-6), 1e32) / radius - l10 * l10;
    const double l11 = sqrt(p1), l21 = (a12 - l20 * l10) / l11;
    const double p2 = a22 + fmin(fmax(a22, 1e-6), 1e32) / radius - l20 * l20 - l21 * l21;
    const double l22 = sqrt(p2);
    bool valid = p0 > 0.0 && p1 > 0.0 && p2 > 0.0 && isfinite(p0) && isfinite(p1) && isfinite(p2);
    const double y0 = -g0 / l00, y1 = (-g1 - l10 * y0) / l11, y2 = (-g2 - l20 * y0 - l21 * y1) / l22;
    const double e2 = y2 / l22, e1 = (y1 - l21 * e2) / l11, e0 = (y0 - l10 * e1 - l20 * e2) / l00;
    const double d[3] = {e0 * sc[0], e1 * sc[1], e2 * sc[2]};
    // the model's cost change -(J d)^T (f + J d / 2) from the sums: -d . g - d^T (J^T J) d / 2
    const double Hd0 = S[0] * d[0] + S[1] * d[1] + S[2] * d[2], Hd1 = S[1] * d[0] + S[3] * d[1] + S[4] * d[2], Hd2 = S[2] * d[0] + S[4] * d[1] + S[5] * d[2];
    const double model = -(d[0] * S[6] + d[1] * S[7] + d[2] * S[8]) - 0.5 * (d[0] * Hd0 + d[1] * Hd1 + d[2] * Hd2);
    valid = valid && isfinite(model) && model > 0.0;
    const bool try_it = valid && !done;
    const double Xt[3] = {try_it ? X[0] + d[0] : X[0], try_it ? X[1] + d[1] : X[1], try_it ? X[2] + d[2] : X[2]};
    double St[10];
    trr_pass<G>(a, r.leaf, tk, l, Xt, St);                // the trial point's cost AND its linearisation
    if (!done) {
      ++it;
      const double cand = St[9];
      if (!valid || !isfinite(cand)) {                   // HandleInvalidStep
        if (++num_invalid >= GSFM_TRR_MAX_INVALID_STEPS) term = GSFM_TERM_FAILURE;
        else { radius /= decrease_factor; decrease_factor *= 2.0; }
        last_successful = false;
      } else {
        num_invalid = 0;
        const double step_norm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), x_norm = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
        const double cost_change = x_cost - cand;
        if (step_norm <= r.parameter_tolerance * (x_norm + r.parameter_tolerance)) term = GSFM_TERM_PARAMETER_TOLERANCE;
        else if (fabs(cost_change) <= r.function_tolerance * x_cost) term = GSFM_TERM_FUNCTION_TOLERANCE;
        else {
          const double rd = cost_change / model;
          if (rd > r.min_relative_decrease) {            // HandleSuccessfulStep: the trial is the next iterate
            X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
#pragma unroll
            for (int k = 0; k < 10; ++k) S[k] = St[k];
            x_cost = cand; gmax = trr_gmax(S);
            const double t = 2.0 * rd - 1.0;
            radius = fmin(r.max_radius, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
            decrease_factor = 2.0;
            last_successful = true;
          } else {                                       // HandleUnsuccessfulStep
            radius /= decrease_factor; decrease_factor *= 2.0;
            last_successful = false;
          }
        }
      }
      if (term < 0) {                                    // the tests at the top of the next iteration
        if (it >= r.max_num_iterations) term = GSFM_TERM_NO_CONVERGENCE;
        else if (last_successful && gmax <= r.gradient_tolerance) term = GSFM_TERM_GRADIENT_TOLERANCE;
        else if (radius <= r.min_radius) term = GSFM_TERM_FAILURE;
      }
      done = term >= 0;
    }
  }
  if (status == 0) {
    if (term == GSFM_TERM_FAILURE) { status = 6; X[0] = 0.0; X[1] = 0.0; X[2] = 0.0; }
    else status = tri_gate<G>(a, tk, l, lane_in_wave, X, n, mean);
  }
  if (tk.live && l == 0) {
    const bool refined = term >= 0;
    a.point[3 * tk.t] = X[0]; a.point[3 * tk.t + 1] = X[1]; a.point[3 * tk.t + 2] = X[2];
    a.status[tk.t] = status;
    a.n_views[tk.t] = n;
    a.mean_sq_err[tk.t] = mean;
    r.iterations[tk.t] = refined ? it : 0;
    r.termination[tk.t] = term;
    r.initial_cost[tk.t] = refined ? initial_cost : 0.0;
    r.final_cost[tk.t] = refined ? x_cost : 0.0;
  }
}

}  // namespace gsfm
