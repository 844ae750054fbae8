// The rule that puts a factorised component of a disconnected view graph to rest (comp_kernels.hpp, k_comp_activity).  Free of HIP headers
// and side effects, so that a host compiler builds it too (tests/cpp/comp_rest_test.cpp checks a table of cases).
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define GSFM_REST_HD __host__ __device__
#else
#define GSFM_REST_HD
#endif

namespace gsfm {

// Trust radius from which the damping D / radius no longer shapes a step: the reference's (Ceres') initial radius, a diagonal shift of 1e-4
// of the clamped Gauss-Newton diagonal.  An absolute statement: it does not move with the caller's initial_trust_region_radius.
#define GSFM_REST_WEAK_DAMPING_RADIUS 1e4

// cur: the component's last exact step (largest camera update, rad), measured at trust radius rad_cur; prev: the one measured before it, at
// rad_prev.  +inf (or NaN) = nothing measured: an idle component, a failed factorisation, the start of a solve.  freeze_below: the rest
// threshold, 0 = never (the MAGSAC losses).  A small step is evidence of convergence only when the damping is not what made it small:
//   * it was measured at a weak damping (rad_cur >= GSFM_REST_WEAK_DAMPING_RADIUS), or
//   * it at least halved against the previous measurement at the same or a growing radius -- steps near convergence contract fast, while a
//     damping-limited step scales with the radius, so a contraction across rejections (radius / 2, / 4, ...) proves nothing.
GSFM_REST_HD inline bool comp_may_rest(double cur, double rad_cur, double prev, double rad_prev, double freeze_below) {
  if (!(freeze_below > 0.0) || !(cur <= freeze_below)) return false;
  if (rad_cur >= GSFM_REST_WEAK_DAMPING_RADIUS) return true;
  return prev <= 1.7976931348623157e308 && cur <= 0.5 * prev && rad_cur >= rad_prev;
}

}  // namespace gsfm
