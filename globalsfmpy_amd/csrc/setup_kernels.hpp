// K0: problem set-up kernels, run once per problem or per weight change: k_build_qrel, k_whiten, the sigma consensus, k_edge_sweep,
// k_row_s, k_gather_weights.  Launched by problem_create.hpp (create, set_edge_weights, sigma consensus) and by launch_row_s in
// solver_launch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"

namespace gsfm {

// ------------------------------------------------------------------------------------------
// K0': measured relative rotations, angle-axis -> unit quaternion planes, gathered into entry order on the device
// (ceres::AngleAxisToQuaternion, estimator.cpp:132; one upload of the 3E doubles instead of a host gather per entry)
__global__ void __launch_bounds__(GSFM_BLOCK) k_build_qrel(const double* __restrict__ rel_aa, const uint32_t* __restrict__ eid, size_t n,
                                                           double2* __restrict__ qr0, double2* __restrict__ qr1, int three) {
  const size_t t = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (t >= n) return;
  const double* aa = rel_aa + 3 * (size_t)eid[t];
  const Quat q = aa_to_quat(aa[0], aa[1], aa[2]);
  if (three) {   // (qrel_three: the W_MATRIX problems)
    double v[3];
    qrel_encode(q, v);
    qr0[t] = make_double2(v[0], v[1]);
    ((double*)qr1)[t] = v[2];
  } else {
    qr0[t] = make_double2(q.x, q.y);
    qr1[t] = make_double2(q.z, q.w);
  }
}

// ------------------------------------------------------------------------------------------
// K0: whitening precompute (src/GSfM_nonlinear_rotation_estimator.cpp:251-288), once per problem
// ------------------------------------------------------------------------------------------
// Lt of cov (already scaled by 1e8): P = cov^-1 by cofactors (Eigen's fixed-size 3x3 inverse), P = L L^T, Lt = L^T (upper triangular:
// l01 = L10, l02 = L20, l12 = L21)
__device__ __forceinline__ EdgeW whitening_factor(double c00, double c11, double c22, double c01, double c02, double c12) {
  const double k00 = c11 * c22 - c12 * c12;
  const double k10 = c12 * c02 - c01 * c22;
  const double k20 = c01 * c12 - c11 * c02;
  const double id = 1.0 / (c00 * k00 + c01 * k10 + c02 * k20);
  const double p00 = k00 * id, p10 = k10 * id, p20 = k20 * id;
  const double p11 = (c00 * c22 - c02 * c02) * id;
  const double p21 = (c02 * c01 - c00 * c12) * id;
  const double p22 = (c00 * c11 - c01 * c01) * id;
  EdgeW W;
  W.l00 = sqrt(p00);
  W.l01 = p10 / W.l00; W.l02 = p20 / W.l00;
  W.l11 = sqrt(p11 - W.l01 * W.l01);
  W.l12 = (p21 - W.l02 * W.l01) / W.l11;
  W.l22 = sqrt(p22 - W.l02 * W.l02 - W.l12 * W.l12);
  return W;
}
struct WhitenArgs {
  const double* cov6;      // per ORIGINAL edge, C00 C11 C22 C01 C02 C12 (may be null)
  const double* inl;       // per original edge (may be null)
  const uint32_t* eid;     // entry -> original edge
  size_t n;
  int error_type;
  double2 *w0, *w1, *w2;   // W_MATRIX outputs
  double* ws;              // W_SCALAR output
};
__global__ void __launch_bounds__(GSFM_BLOCK) k_whiten(WhitenArgs a) {
  const size_t t = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (t >= a.n) return;
  const size_t e = a.eid[t];
  double cov[6] = {0, 0, 0, 0, 0, 0};
  if (a.cov6) {
#pragma unroll
    for (int k = 0; k < 6; ++k) cov[k] = a.cov6[6 * e + k] * 1e8;  // :252
  }
  const double iw = a.inl ? a.inl[e] : 1.0;
  const double c00 = cov[0], c11 = cov[1], c22 = cov[2], c01 = cov[3], c02 = cov[4], c12 = cov[5];
  if (a.error_type == GSFM_ROT_ANGLE_AXIS_COVARIANCE || a.error_type == GSFM_ROT_ANGLE_AXIS_COV_INLIERS) {
    const EdgeW W = whitening_factor(c00, c11, c22, c01, c02, c12);
    const double m = (a.error_type == GSFM_ROT_ANGLE_AXIS_COV_INLIERS) ? iw : 1.0;
    a.w0[t] = make_double2(W.l00 * m, W.l01 * m);
    a.w1[t] = make_double2(W.l02 * m, W.l11 * m);
    a.w2[t] = make_double2(W.l12 * m, W.l22 * m);
  } else if (a.error_type == GSFM_ROT_ANGLE_AXIS_INLIERS) {
    a.ws[t] = iw;                                                     // :263
  } else if (a.error_type == GSFM_ROT_ANGLE_AXIS_COVTRACE) {
    a.ws[t] = sqrt(1.0 / (c00 + c11 + c22));                          // :276-281
  } else if (a.error_type == GSFM_ROT_ANGLE_AXIS_COVNORM) {
    const double f = c00 * c00 + c11 * c11 + c22 * c22 + 2.0 * (c01 * c01 + c02 * c02 + c12 * c12);
    a.ws[t] = sqrt(1.0 / sqrt(f));                                    // :284-286
  }
}

// sigma-consensus weights (src/GSfM_nonlinear_rotation_estimator.cpp:400-416).  The weight of an edge depends only on its UNWEIGHTED
// residual at the rotations an outer iteration starts from -- exactly the point the inner solve's first cost sweep (K1) and first
// linearisation (K2) evaluate anyway.  So there is no weight pass: in `sigma` mode K1 and K2 compute the weight from the unit-weight
// residual they have in registers, store it into their own scalar-weight plane in their own order (8 B per edge / directed entry,
// coalesced) and use it at once; K1 also sums |w - w_old| against the plane's previous content.  Later sweeps of the solve read the
// planes as usual.  (Round 2: an s-only sweep, a weight kernel over the original edge order and two scattered gathers, 478 us at C5.)
struct SigmaDev {
  const double* table;    // Gamma(1, x / 1000), nu = 3
  int table_len;
  int on;                 // 1: this launch computes and stores the weights
  double ssm2, one_over_sigma, gk, weight_zero;
  double inv_ssm2;        // 1 / ssm2 (the fast path of sigma_weight)
};
// The reference's arithmetic -- residual = sqrt(s), squared_residual = residual * residual, x = round(1000 * squared_residual / ssm2) -- costs a
// correctly rounded fp64 square root and division per edge (~45 VALU instructions: the sweep is issue-bound, round-4 SQ counters) for the sake
// of an INTEGER: the table cell.  Round 5: the cell is taken from t = 1000 s / ssm2 evaluated with one multiplication by the reciprocal,
// which is within a few ulp of the reference's argument of round() (sqrt-then-square moves s by at most 2 ulp, the reciprocal by 1.5), so it
// names the same cell unless t lies within ~1e-15 t of a half-integer; lanes closer than 1e-12 t to one (and the ones at the zero-residual
// test) redo it the reference's way.  Same cell -> the same table entry -> the same weight, bit for bit (tests/test_gpu_round3.py).
__device__ __forceinline__ double sigma_weight(const SigmaDev& g, double s_unit) {
  const double last = (double)(g.table_len - 1);
  const double t = 1000.0 * s_unit * g.inv_ssm2;
  double xf = round(t);                                                  // std::round: halves away from zero
  const double frac = fabs(t - xf);                                      // distance to the nearest integer: 0.5 at a cell boundary
  const bool sure = s_unit > 1e-30 && (t > last + 1.0 || fabs(frac - 0.5) > 1e-12 * fmax(t, 1.0));
  if (!sure) {
    const double residual = sqrt(s_unit);
    if (residual < 2.220446049250313e-16) return g.weight_zero;
    const double squared_residual = residual * residual;                 // as written in the reference, not s itself
    xf = round(1000.0 * squared_residual / g.ssm2);
  }
  if (!(xf < last)) xf = last;                                           // last stored entry (the reference reads one past it)
  return g.one_over_sigma * (g.table[(int)xf] - g.gk);
}

// The step after the solve and the evaluation statistic as one edge sweep with K1's device routines, without a problem object:
//   FilterViewPairsFromOrientation (Theia filter_view_pairs_from_orientation.cc:55-122): s_e = |log(R_ij^T R_j R_i^T)|^2 against a threshold;
//   residuals_of_relative_rot (src/compare_reconstructions.cpp:617-647): s_e = |Lt log(R_j R_i^T R_ij^T)|^2 with Lt from 1e8 Sigma_e.
// One edge per lane, edges in the caller's order (coalesced 8 + 24 (+ 48) B per edge in, 8 (+ 1) B out), camera quaternions gathered.
struct EdgeSweepArgs {
  size_t n;
  const uint32_t *ei, *ej;
  const double* rel_aa;   // 3 per edge
  const double* cov6;     // 6 per edge or null (unweighted)
  const double2* q;       // camera quaternion cache
  double max_sq;          // keep = s <= max_sq (ignored when keep is null)
  double* s_out;
  uint8_t* keep;
  unsigned long long* n_kept;
};
__global__ void __launch_bounds__(GSFM_BLOCK) k_edge_sweep(EdgeSweepArgs a) {
  const size_t e = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  bool kept = false;
  if (e < a.n) {
    const Quat qi = load_q(a.q, a.ei[e]), qj = load_q(a.q, a.ej[e]);
    const Quat qr = aa_to_quat(a.rel_aa[3 * e], a.rel_aa[3 * e + 1], a.rel_aa[3 * e + 2]);
    double r[3];
    if (a.cov6) {
      const double* c = a.cov6 + 6 * e;
      const EdgeW W = whitening_factor(c[0] * 1e8, c[1] * 1e8, c[2] * 1e8, c[3] * 1e8, c[4] * 1e8, c[5] * 1e8);
      edge_residual<F_AA, W_MATRIX>(qi, qj, qr, W, r);
    } else {
      EdgeW W;
      W.l00 = 1.0; W.l01 = W.l02 = W.l12 = 0.0; W.l11 = W.l22 = 1.0;
      edge_residual<F_AA, W_NONE>(qi, qj, qr, W, r);
    }
    const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    a.s_out[e] = s;
    kept = s <= a.max_sq;
    if (a.keep) a.keep[e] = kept ? 1 : 0;
  }
  if (a.keep) {   // integer count: order-independent, so an atomic is exact
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.n_kept, (unsigned long long)__popcll(b));
  }
}

// s = |r_e|^2 of EVERY edge a rank holds (each touches one of its rows), written per local edge, by rows of the block-CSR: on a sharded
// problem the cost sweep K1 only visits the edges a rank counts in the cost, but sigma consensus (unit weights, UNIT = true) and
// host-callback losses (the problem's own whitening) need s for both ends' rows.  Same device routine as K1, so two ranks holding the
// same edge -- and the single-GPU sweep -- produce the same bits.
struct RowSArgs {
  uint32_t n_rows, row_base, G;
  const uint32_t* row_ptr;
  const uint32_t* col;
  const uint32_t* eid;
  const double2 *qr0, *qr1;
  const double2 *w0, *w1, *w2;
  const double* ws;
  const double2* q;
  double* s_out;          // per local edge
};
template <int F, int WM, bool UNIT>
__global__ void __launch_bounds__(GSFM_BLOCK) k_row_s(RowSArgs a) {
  constexpr int R = ResDim<F>::R;
  const uint32_t t = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const uint32_t row = t / a.G, lane = t % a.G;
  if (row >= a.n_rows) return;
  const Quat qk = load_q(a.q, a.row_base + row);
  const uint32_t end = a.row_ptr[row + 1];
  for (uint32_t d = a.row_ptr[row] + lane; d < end; d += a.G) {
    const uint32_t cr = a.col[d];
    const Quat qm = load_q(a.q, cr & 0x7fffffffu);
    double2 r0, r1;
    qrel_load<WM>(a.qr0, a.qr1, d, r0, r1);
    const Quat qr = qrel_quat<WM>(r0, r1);
    EdgeW W = load_w<WM>(a.w0, a.w1, a.w2, a.ws, d);
    if (UNIT) W.l00 = 1.0;
    double r[R];
    if (cr >> 31) edge_residual<F, WM>(qm, qk, qr, W, r);
    else edge_residual<F, WM>(qk, qm, qr, W, r);
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < R; ++c) s += r[c] * r[c];
    a.s_out[a.eid[d]] = s;
  }
}

// scatter per-original-edge scalar weights into an entry-ordered plane (sigma consensus / set_edge_weights)
__global__ void __launch_bounds__(GSFM_BLOCK) k_gather_weights(const double* __restrict__ w_orig,
                                                               const uint32_t* __restrict__ eid, size_t n,
                                                               double* __restrict__ ws) {
  const size_t t = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (t < n) ws[t] = w_orig[eid[t]];
}

}  // namespace gsfm
