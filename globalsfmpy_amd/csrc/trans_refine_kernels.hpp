// Device kernel of the relative-translation refinement (include/gsfm_pos.h, gsfm_pos_refine_relative_translations): Theia's
// OptimizeRelativePositionWithKnownRotation for every view pair, under the definition of that header.
//
// ONE WAVEFRONT owns one edge (the shape of k_cov_estimate): the 64 lanes stride over the edge's matches, the seven sums of an IRLS
// iteration (six entries of L and the cost) are reduced with the fixed xor-butterfly wave_allsum, so every lane holds the same values,
// and all lanes run the 3 x 3 eigen-solve and the loop control redundantly.  No LDS, no atomics, nothing waits for another workgroup
// and the host is not asked anything inside the loop.  The sums are taken in a fixed order (lane l adds matches l, l + 64, ... in that
// order, then the butterfly), and an edge's arithmetic depends on nothing but that edge: two calls return the same bytes, and so does a
// call with the edges in another order.
//
// Passes over an edge's matches:
//   pass 0      features -> constraint a_m, stored once to a structure-of-arrays plane (ax | ay | az, 24 B per match), and L_0 (w = 1);
//   pass k >= 1 w = |t_{k-1} . a_m| from the plane: cost_{k-1} = sum w and L_k = sum a a^T / max(w, 1e-7) TOGETHER -- the weights are
//               never stored.  delta_{k-1} and with it the stopping test of iteration k-1 are known after pass k, so the last pass's
//               L is computed and dropped: iterations + 1 passes in place of 2 x iterations, the same deltas and the same count;
//   last pass   the in-front count from the pixel records and the sign.
// A lane re-reads only what it wrote itself to the plane (the same stride in every pass), so no fence is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cov_kernels.hpp"

namespace gsfm {

#define GSFM_TR_MAX_ITERATIONS 100
#define GSFM_TR_MAX_INNER 10
#define GSFM_TR_EPS 1e-5
#define GSFM_TR_MIN_WEIGHT 1e-7
#define GSFM_TR_JACOBI_SWEEPS 16

struct TrArgs {
  uint64_t n_edges;
  uint64_t n_matches;          // the stride of the constraint plane
  const uint32_t* order;       // launch slot -> edge (descending match count), outputs stay in caller order
  const uint32_t* edge_i;
  const uint32_t* edge_j;
  const uint64_t* match_ptr;   // [n_edges + 1]
  const double4* matches;      // x1 y1 x2 y2 (pixels)
  const double* intr;          // f1 u1 v1 f2 u2 v2 per edge
  const double* rot_aa;        // 3 per camera
  const double* rel_t_in;      // 3 per edge
  double* plane;               // 3 x n_matches: ax | ay | az
  double* rel_t_out;
  int32_t* status;             // 0 refined, 1 skipped (fewer than 2 matches), 2 non-finite
  int32_t* iters;
  double* cost;
};

// Unit eigenvector of the smallest eigenvalue of the symmetric 3 x 3 matrix (xx xy xz yy yz zz), which the caller has divided by its
// trace.  Cyclic Jacobi in fp64: sweeps over the pairs (0,1), (0,2), (1,2); a pair is rotated when |a_pq| > 2^-54 sqrt(|a_pp a_qq|)
// (the relative criterion for definite matrices: below it the rotation changes neither diagonal entry's last bit); the solve stops at
// the first sweep that rotates no pair, after GSFM_TR_JACOBI_SWEEPS sweeps at the latest (a 3 x 3 needs 4 to 6).  Among equal
// eigenvalues the lowest index.  The column is normalised once more, so |t| = 1 to rounding.
__device__ __forceinline__ void tr_smallest_eigenvector(const double* L, double* t) {
  double a00 = L[0], a01 = L[1], a02 = L[2], a11 = L[3], a12 = L[4], a22 = L[5];
  double v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // row-major, columns = eigenvectors
#define GSFM_TR_ROTATE(app, aqq, apq, arp, arq, P, Q)                                         \
  if (fabs(apq) > 5.551115123125783e-17 * sqrt(fabs(app * aqq))) {                            \
    const double theta = (aqq - app) / (2.0 * apq);                                           \
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));       \
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;                                   \
    app -= tt * apq; aqq += tt * apq; apq = 0.0;                                              \
    const double rp = arp, rq = arq;                                                          \
    arp = c * rp - s * rq; arq = s * rp + c * rq;                                             \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                           \
      const double vp = v[3 * r + P], vq = v[3 * r + Q];                                      \
      v[3 * r + P] = c * vp - s * vq; v[3 * r + Q] = s * vp + c * vq;                         \
    }                                                                                         \
    rotated = true;                                                                           \
  }
  for (int sweep = 0; sweep < GSFM_TR_JACOBI_SWEEPS; ++sweep) {
    bool rotated = false;
    GSFM_TR_ROTATE(a00, a11, a01, a02, a12, 0, 1)
    GSFM_TR_ROTATE(a00, a22, a02, a01, a12, 0, 2)
    GSFM_TR_ROTATE(a11, a22, a12, a01, a02, 1, 2)
    if (!rotated) break;
  }
#undef GSFM_TR_ROTATE
  int col = 0;
  double lo = a00;
  if (a11 < lo) { lo = a11; col = 1; }
  if (a22 < lo) { lo = a22; col = 2; }
  const double x = col == 0 ? v[0] : col == 1 ? v[1] : v[2];
  const double y = col == 0 ? v[3] : col == 1 ? v[4] : v[5];
  const double z = col == 0 ? v[6] : col == 1 ? v[7] : v[8];
  const double nrm = sqrt(x * x + y * y + z * z);
  t[0] = x / nrm; t[1] = y / nrm; t[2] = z / nrm;
}

__device__ __forceinline__ void tr_mat_vec(const double* R, const double* x, double* y) {      // y = R x
#pragma unroll
  for (int r = 0; r < 3; ++r) y[r] = R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2];
}
__device__ __forceinline__ void tr_mat_t_vec(const double* R, const double* x, double* y) {    // y = R^T x
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = R[c] * x[0] + R[3 + c] * x[1] + R[6 + c] * x[2];
}

__global__ void __launch_bounds__(64) k_tr_refine(TrArgs a) {
  if (blockIdx.x >= a.n_edges) return;
  const uint64_t e = a.order[blockIdx.x];
  const int lane = threadIdx.x;
  const uint64_t mb = a.match_ptr[e], me = a.match_ptr[e + 1], n = me - mb;
  double t[3] = {a.rel_t_in[3 * e], a.rel_t_in[3 * e + 1], a.rel_t_in[3 * e + 2]};
  int status = 0, it = 0;
  double cost = 0.0;
  if (n < 2) status = 1;
  else {
    double K[6], R1[9], R2[9], w1[3], w2[3];
    const uint32_t ci = a.edge_i[e], cj = a.edge_j[e];
#pragma unroll
    for (int k = 0; k < 6; ++k) K[k] = a.intr[6 * e + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { w1[k] = a.rot_aa[3 * (uint64_t)ci + k]; w2[k] = a.rot_aa[3 * (uint64_t)cj + k]; }
    rodrigues(w1, R1);
    rodrigues(w2, R2);
    double* const px = a.plane, * const py = a.plane + a.n_matches, * const pz = a.plane + 2 * a.n_matches;
    // ---- pass 0: the constraints, once, and L_0 (all weights 1) ----
    double s[7] = {0, 0, 0, 0, 0, 0, 0};   // xx xy xz yy yz zz, cost
    for (uint64_t k = mb + lane; k < me; k += 64) {
      const double4 m = a.matches[k];
      const double f1[3] = {(m.x - K[1]) / K[0], (m.y - K[2]) / K[0], 1.0};
      const double f2[3] = {(m.z - K[4]) / K[3], (m.w - K[5]) / K[3], 1.0};
      double r1[3], r2[3], c[3];
      tr_mat_t_vec(R1, f1, r1);
      tr_mat_t_vec(R2, f2, r2);
      const double cr[3] = {r2[1] * r1[2] - r2[2] * r1[1], r2[2] * r1[0] - r2[0] * r1[2], r2[0] * r1[1] - r2[1] * r1[0]};
      tr_mat_vec(R1, cr, c);
      px[k] = c[0]; py[k] = c[1]; pz[k] = c[2];
      s[0] += c[0] * c[0]; s[1] += c[0] * c[1]; s[2] += c[0] * c[2]; s[3] += c[1] * c[1]; s[4] += c[1] * c[2]; s[5] += c[2] * c[2];
    }
    double L[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) L[k] = wave_allsum(s[k]);
    // ---- IRLS ----
    int inner = 0;
    double tn[3] = {t[0], t[1], t[2]};
    while (true) {
      const double tr = L[0] + L[3] + L[5];
      if (!(tr > 0.0) || !isfinite(tr)) { status = 2; break; }   // all-zero constraints or non-finite input
#pragma unroll
      for (int k = 0; k < 6; ++k) L[k] /= tr;
      tr_smallest_eigenvector(L, tn);
#pragma unroll
      for (int k = 0; k < 7; ++k) s[k] = 0.0;
      for (uint64_t k = mb + lane; k < me; k += 64) {
        const double c0 = px[k], c1 = py[k], c2 = pz[k];
        const double w = fabs(tn[0] * c0 + tn[1] * c1 + tn[2] * c2);
        s[6] += w;                                               // the cost takes the unfloored weight
        const double inv = 1.0 / fmax(w, GSFM_TR_MIN_WEIGHT);
        const double b0 = c0 * inv, b1 = c1 * inv, b2 = c2 * inv;
        s[0] += b0 * c0; s[1] += b0 * c1; s[2] += b0 * c2; s[3] += b1 * c1; s[4] += b1 * c2; s[5] += b2 * c2;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) L[k] = wave_allsum(s[k]);
      const double new_cost = wave_allsum(s[6]);
      const double delta = fmax(fabs(cost - new_cost), 1.0 - (tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]));
      inner = (delta <= GSFM_TR_EPS) ? inner + 1 : 0;
      cost = new_cost;
      ++it;
      if (it >= GSFM_TR_MAX_ITERATIONS || inner >= GSFM_TR_MAX_INNER) break;
    }
    if (status == 0 && !(isfinite(tn[0]) && isfinite(tn[1]) && isfinite(tn[2]) && isfinite(cost))) status = 2;
    if (status == 0) {
      // ---- the sign: negate unless more than n / 2 matches lie in front of both cameras ----
      unsigned long long in_front = 0;
      for (uint64_t k0 = mb; k0 < me; k0 += 64) {
        const uint64_t k = k0 + lane;
        bool ok = false;
        if (k < me) {
          const double4 m = a.matches[k];
          const double d1[3] = {(m.x - K[1]) / K[0], (m.y - K[2]) / K[0], 1.0};
          const double f2[3] = {(m.z - K[4]) / K[3], (m.w - K[5]) / K[3], 1.0};
          double r2[3], d2[3];
          tr_mat_t_vec(R2, f2, r2);
          tr_mat_vec(R1, r2, d2);                                // Rrel^T f2, Rrel = R2 R1^T
          const double d11 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], d22 = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
          const double d12 = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
          const double d1t = d1[0] * tn[0] + d1[1] * tn[1] + d1[2] * tn[2], d2t = d2[0] * tn[0] + d2[1] * tn[1] + d2[2] * tn[2];
          ok = (d22 * d1t - d12 * d2t > 0.0) && (d12 * d1t - d11 * d2t > 0.0);
        }
        in_front += (unsigned long long)__popcll(__ballot(ok));
      }
      const double sg = (in_front > n / 2) ? 1.0 : -1.0;
      t[0] = sg * tn[0]; t[1] = sg * tn[1]; t[2] = sg * tn[2];
    }
  }
  if (lane == 0) {
    a.rel_t_out[3 * e] = t[0]; a.rel_t_out[3 * e + 1] = t[1]; a.rel_t_out[3 * e + 2] = t[2];
    a.status[e] = status;
    a.iters[e] = status == 1 ? 0 : it;
    a.cost[e] = status == 0 ? cost : 0.0;
  }
}

}  // namespace gsfm
