// Device kernels of camera-position estimation (include/gsfm_pos.h): the reference's EstimatePositions with BASELINE residuals,
// r = (c_j - c_i) / |c_j - c_i| - R_i^T t_ij, one robust residual per view-graph edge, one 3-vector per camera.
//
// Layout.  Every edge appears twice in a per-camera CSR of directed entries (row k, neighbour m, neighbours sorted within a row, repeated
// pairs in edge order).  An entry stores its edge's world direction with the sign of its own end applied -- +d on the i-side, -d on the
// j-side -- so that from row k the residual reads r_k = w / |w| - d_k with w = c_m - c_k, which is +r_e on the i-side and -r_e on the
// j-side, to the bit (IEEE subtraction and division are sign-symmetric).  Both entries of an edge therefore compute the same rho, the same
// Corrector and the same block H_e = J~^T J~; the two Jacobians of an edge are -J~ (row k) and +J~ (neighbour), so the normal matrix is a
// block graph Laplacian: diagonal D_k = sum H_e, off-diagonal -H_e, and  (L p)_k = sum_{e at k} H_e (p_k - p_m).
// The blocks are kept unscaled; Jacobi scaling S and the LM damping are applied as vector operations around the product.
//
// Determinism: one wavefront per row, lanes stride the row, a fixed shuffle tree per row; every global sum runs over a fixed number of
// partials in a fixed order.  No atomics anywhere.  Two solves of the same input give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "loss_dev.hpp"
#include "edge_math.hpp"
#include "dense_assemble_kernels.hpp"

namespace gsfm {

#define GSFM_POS_PARTS 512           // partials of every vector reduction (a constant: the order of each sum does not depend on the run)
enum { POS_LM_EXT = 3 };             // rho triples supplied per edge by the host (callback loss); otherwise LM_SIMPLE / LM_PROGRAM

struct PosDev {
  uint32_t n_cams;
  uint32_t n_edges;
  const uint32_t* row_ptr;   // N + 1
  const uint32_t* nbr;       // 2E: neighbour of each directed entry
  const uint32_t* eid;       // 2E: edge of each directed entry (read by the callback-loss path only)
  const double* dir_k;       // 2E x 3: the edge's world direction with this end's sign
  const uint32_t* ei;        // E
  const uint32_t* ej;        // E
  const double* dir_e;       // E x 3: d_e = R(aa_i)^T position_2
  const uint8_t* active;     // N: 1 = a free parameter block (has an edge, is not the fixed camera)
  double* H;                 // 2E x 6: H_e of each entry (00 01 02 11 12 22), written by the linearisation
  const DevLoss* loss;
  const double* rho_ext;     // E x 3 (callback loss)
};

// r = w / n - d with n = |w|, n := 1 below 1e-12 (the reference's guard).  unit: n was kept, i.e. dr/dc_m = (I - u u^T) / n, else I.
__device__ __forceinline__ bool pos_residual(double w0, double w1, double w2, const double* d, double* r, double* u, double& n) {
  n = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const bool unit = !(n < 1e-12);
  if (!unit) n = 1.0;
  u[0] = w0 / n; u[1] = w1 / n; u[2] = w2 / n;
  r[0] = u[0] - d[0]; r[1] = u[1] - d[1]; r[2] = u[2] - d[2];
  return unit;
}

template <int LM>
__device__ __forceinline__ Rho3 pos_rho(const PosDev& a, uint32_t e, double s) {
  if (LM == POS_LM_EXT) { Rho3 o; o.r0 = a.rho_ext[3 * (size_t)e]; o.r1 = a.rho_ext[3 * (size_t)e + 1]; o.r2 = a.rho_ext[3 * (size_t)e + 2]; return o; }
  return loss_eval<LM == LM_SIMPLE ? LM_SIMPLE : LM_PROGRAM>(a.loss, s);
}

// Linearisation: per directed entry the corrected Jacobian A = C P (C = sqrt(rho') (I - alpha r r^T / ...), Ceres' Corrector), its block
// H = A^T A (stored), and the row's gradient g_k = sum -A^T r~ and diagonal block D_k = sum H, reduced per wavefront in a fixed order.
template <int LM>
__global__ void __launch_bounds__(256) k_pos_lin(PosDev a, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  const double xk0 = x[3 * (size_t)row], xk1 = x[3 * (size_t)row + 1], xk2 = x[3 * (size_t)row + 2];
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t end = a.row_ptr[row + 1];
  for (uint32_t d = a.row_ptr[row] + lane; d < end; d += 64) {
    const uint32_t m = a.nbr[d];
    double r[3], u[3], n;
    const bool unit = pos_residual(x[3 * (size_t)m] - xk0, x[3 * (size_t)m + 1] - xk1, x[3 * (size_t)m + 2] - xk2, a.dir_k + 3 * (size_t)d, r, u, n);
    const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const Rho3 rho = pos_rho<LM>(a, LM == POS_LM_EXT ? a.eid[d] : 0u, s);
    const Corrector c = make_corrector(s, rho);
    double A[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) A[3 * i + j] = unit ? ((i == j ? 1.0 : 0.0) - u[i] * u[j]) / n : (i == j ? 1.0 : 0.0);
    if (c.alpha_sq_norm == 0.0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) A[k] *= c.sqrt_rho1;
    } else {
#pragma unroll
      for (int col = 0; col < 3; ++col) {
        const double t = r[0] * A[col] + r[1] * A[3 + col] + r[2] * A[6 + col];
#pragma unroll
        for (int k = 0; k < 3; ++k) A[3 * k + col] = c.sqrt_rho1 * (A[3 * k + col] - c.alpha_sq_norm * r[k] * t);
      }
    }
    const double rt0 = c.residual_scaling * r[0], rt1 = c.residual_scaling * r[1], rt2 = c.residual_scaling * r[2];
#pragma unroll
    for (int col = 0; col < 3; ++col) acc[col] -= A[col] * rt0 + A[3 + col] * rt1 + A[6 + col] * rt2;
    double h[6];
    h[0] = A[0] * A[0] + A[3] * A[3] + A[6] * A[6];
    h[1] = A[0] * A[1] + A[3] * A[4] + A[6] * A[7];
    h[2] = A[0] * A[2] + A[3] * A[5] + A[6] * A[8];
    h[3] = A[1] * A[1] + A[4] * A[4] + A[7] * A[7];
    h[4] = A[1] * A[2] + A[4] * A[5] + A[7] * A[8];
    h[5] = A[2] * A[2] + A[5] * A[5] + A[8] * A[8];
    double2* hp = (double2*)(a.H + 6 * (size_t)d);
    hp[0] = make_double2(h[0], h[1]); hp[1] = make_double2(h[2], h[3]); hp[2] = make_double2(h[4], h[5]);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[3 + k] += h[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    for (int k = 0; k < 3; ++k) g[3 * (size_t)row + k] = acc[k];
    for (int k = 0; k < 6; ++k) Dg[6 * (size_t)row + k] = acc[3 + k];
  }
}

// sum over edges of rho(s_e) / 2 at x: GSFM_POS_PARTS workgroups stride the edges, one partial each
template <int LM>
__global__ void __launch_bounds__(256) k_pos_cost(PosDev a, const double* __restrict__ x, double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < a.n_edges; e += (size_t)GSFM_POS_PARTS * 256) {
    const uint32_t i = a.ei[e], j = a.ej[e];
    double r[3], u[3], n;
    pos_residual(x[3 * (size_t)j] - x[3 * (size_t)i], x[3 * (size_t)j + 1] - x[3 * (size_t)i + 1], x[3 * (size_t)j + 2] - x[3 * (size_t)i + 2], a.dir_e + 3 * e, r, u, n);
    const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    acc += 0.5 * loss_value<LM == LM_SIMPLE ? LM_SIMPLE : LM_PROGRAM>(a.loss, s);
  }
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// per edge: residual, squared norm and (in-kernel loss) rho; for gsfm_pos_residuals and for the host-callback loss
__global__ void __launch_bounds__(256) k_pos_resid(PosDev a, const double* __restrict__ x, double* __restrict__ r_out, double* __restrict__ s_out,
                                                   double* __restrict__ rho_out, int in_kernel_loss) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_edges) return;
  const uint32_t i = a.ei[e], j = a.ej[e];
  double r[3], u[3], n;
  pos_residual(x[3 * (size_t)j] - x[3 * (size_t)i], x[3 * (size_t)j + 1] - x[3 * (size_t)i + 1], x[3 * (size_t)j + 2] - x[3 * (size_t)i + 2], a.dir_e + 3 * e, r, u, n);
  const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  if (r_out) { r_out[3 * e] = r[0]; r_out[3 * e + 1] = r[1]; r_out[3 * e + 2] = r[2]; }
  if (s_out) s_out[e] = s;
  if (rho_out && in_kernel_loss) rho_out[e] = loss_eval<LM_PROGRAM>(a.loss, s).r0;
}

// y_k = sum_e H_e (q_k - q_m).  SCALED: the PCG operator in Jacobi-scaled coordinates, out = S (L (S p)) + D^2 p with q = S p given, and
// the identity on inactive rows; otherwise out = L q (0 on inactive rows).
template <bool SCALED>
__global__ void __launch_bounds__(256) k_pos_matvec(PosDev a, const double* __restrict__ q, const double* __restrict__ p, const double* __restrict__ S,
                                                    const double* __restrict__ D2, double* __restrict__ out) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t k3 = 3 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 3) out[k3 + lane] = SCALED ? p[k3 + lane] : 0.0;
    return;
  }
  const double q0 = q[k3], q1 = q[k3 + 1], q2 = q[k3 + 2];
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  const uint32_t end = a.row_ptr[row + 1];
  for (uint32_t d = a.row_ptr[row] + lane; d < end; d += 64) {
    const uint32_t m = a.nbr[d];
    const double2* hp = (const double2*)(a.H + 6 * (size_t)d);
    const double2 h01 = hp[0], h23 = hp[1], h45 = hp[2];
    const double v0 = q0 - q[3 * (size_t)m], v1 = q1 - q[3 * (size_t)m + 1], v2 = q2 - q[3 * (size_t)m + 2];
    y0 += h01.x * v0 + h01.y * v1 + h23.x * v2;
    y1 += h01.y * v0 + h23.y * v1 + h45.x * v2;
    y2 += h23.x * v0 + h45.x * v1 + h45.y * v2;
  }
  y0 = wave_sum(y0); y1 = wave_sum(y1); y2 = wave_sum(y2);
  if (lane == 0) {
    if (SCALED) {
      out[k3] = S[k3] * y0 + D2[k3] * p[k3];
      out[k3 + 1] = S[k3 + 1] * y1 + D2[k3 + 1] * p[k3 + 1];
      out[k3 + 2] = S[k3 + 2] * y2 + D2[k3 + 2] * p[k3 + 2];
    } else { out[k3] = y0; out[k3 + 1] = y1; out[k3 + 2] = y2; }
  }
}

// ---- reductions: GSFM_POS_PARTS partials, then one workgroup -------------------------------------------------------------------
// sum_i a_i b_i over n = 3 N entries (mask: per camera, may be NULL)
__global__ void __launch_bounds__(256) k_pos_dot(const double* __restrict__ a, const double* __restrict__ b, const uint8_t* __restrict__ mask, size_t n,
                                                 double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)GSFM_POS_PARTS * 256)
    if (!mask || mask[i / 3]) acc += a[i] * b[i];
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256) k_pos_absmax(const double* __restrict__ a, const uint8_t* __restrict__ mask, size_t n, double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)GSFM_POS_PARTS * 256)
    if (!mask || mask[i / 3]) acc = fmax(acc, fabs(a[i]));   // (a NaN entry is dropped: fmax(acc, NaN) = acc, as std::fmax in the oracle)
  const double t = block_max_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256) k_pos_reduce(const double* __restrict__ part, double* __restrict__ out, int is_max) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (int k = threadIdx.x; k < GSFM_POS_PARTS; k += 256) acc = is_max ? fmax(acc, part[k]) : acc + part[k];
  const double t = is_max ? block_max_bcast(acc, lds) : block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) *out = t;
}

// Jacobi scaling from the first linearisation: S = 1 / (1 + sqrt(column norm^2)) (Ceres: computed once, at the start point)
__global__ void k_pos_scale(uint32_t n_cams, const double* __restrict__ Dg, double* __restrict__ S, int jacobi) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double* D = Dg + 6 * (size_t)k;
  S[3 * (size_t)k] = jacobi ? 1.0 / (1.0 + sqrt(D[0])) : 1.0;
  S[3 * (size_t)k + 1] = jacobi ? 1.0 / (1.0 + sqrt(D[3])) : 1.0;
  S[3 * (size_t)k + 2] = jacobi ? 1.0 / (1.0 + sqrt(D[5])) : 1.0;
}

// inverse of a symmetric 3x3 (m: 00 01 02 11 12 22) by cofactors, all nine entries
__device__ __forceinline__ void pos_inv3(const double* m, double* o) {
  const double c00 = m[3] * m[5] - m[4] * m[4], c01 = m[2] * m[4] - m[1] * m[5], c02 = m[1] * m[4] - m[2] * m[3];
  const double c11 = m[0] * m[5] - m[2] * m[2], c12 = m[1] * m[2] - m[0] * m[4], c22 = m[0] * m[3] - m[1] * m[1];
  const double inv = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * inv; o[1] = c01 * inv; o[2] = c02 * inv;
  o[3] = c01 * inv; o[4] = c11 * inv; o[5] = c12 * inv;
  o[6] = c02 * inv; o[7] = c12 * inv; o[8] = c22 * inv;
}

// Start of a step: D^2 = clamp(S^2 diag(D_k)) / radius (LevenbergMarquardtStrategy), the right-hand side b = S g, the scaled damped
// diagonal blocks M_k = S D_k S + D^2 (kept for the dense assembly) and their inverses, and the PCG start y = 0, r = b, z = M^-1 r, p = z,
// q = S p.  Inactive rows: M = I, everything else 0.
__global__ void k_pos_prep(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ Dg, const double* __restrict__ g,
                           const double* __restrict__ S, double radius, double min_diag, double max_diag, double* __restrict__ D2,
                           double* __restrict__ Mblk, double* __restrict__ Minv, double* __restrict__ b, double* __restrict__ r, double* __restrict__ z,
                           double* __restrict__ p, double* __restrict__ q, double* __restrict__ y) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t k3 = 3 * (size_t)k;
  double M[6] = {1, 0, 0, 1, 0, 1}, Mi[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, bb[3] = {0, 0, 0}, dd[3] = {0, 0, 0};
  if (active[k]) {
    const double* D = Dg + 6 * (size_t)k;
    const double s0 = S[k3], s1 = S[k3 + 1], s2 = S[k3 + 2];
    const double sc[3] = {s0, s1, s2};
    const double dg[3] = {D[0], D[3], D[5]};
    for (int c = 0; c < 3; ++c) dd[c] = fmin(fmax(sc[c] * sc[c] * dg[c], min_diag), max_diag) / radius;
    M[0] = s0 * D[0] * s0 + dd[0]; M[1] = s0 * D[1] * s1; M[2] = s0 * D[2] * s2;
    M[3] = s1 * D[3] * s1 + dd[1]; M[4] = s1 * D[4] * s2; M[5] = s2 * D[5] * s2 + dd[2];
    pos_inv3(M, Mi);
    for (int c = 0; c < 3; ++c) bb[c] = sc[c] * g[k3 + c];
  }
  for (int c = 0; c < 3; ++c) {
    D2[k3 + c] = dd[c]; b[k3 + c] = bb[c]; r[k3 + c] = bb[c]; y[k3 + c] = 0.0;
    const double zc = Mi[3 * c] * bb[0] + Mi[3 * c + 1] * bb[1] + Mi[3 * c + 2] * bb[2];
    z[k3 + c] = zc; p[k3 + c] = zc; q[k3 + c] = active[k] ? S[k3 + c] * zc : 0.0;
  }
  for (int c = 0; c < 6; ++c) Mblk[6 * (size_t)k + c] = M[c];
  for (int c = 0; c < 9; ++c) Minv[9 * (size_t)k + c] = Mi[c];
}

// PCG: y += alpha p, r -= alpha A p, z = M^-1 r with alpha = rz / pAp from the device scalars
__global__ void k_pos_pcg_update(uint32_t n_cams, const double* __restrict__ scal, int s_rz, int s_pap, const double* __restrict__ p,
                                 const double* __restrict__ Ap, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z,
                                 const double* __restrict__ Minv) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double pap = scal[s_pap];
  const double alpha = pap > 0.0 ? scal[s_rz] / pap : 0.0;
  const size_t k3 = 3 * (size_t)k;
  double rr[3];
  for (int c = 0; c < 3; ++c) { y[k3 + c] += alpha * p[k3 + c]; rr[c] = r[k3 + c] - alpha * Ap[k3 + c]; r[k3 + c] = rr[c]; }
  const double* Mi = Minv + 9 * (size_t)k;
  for (int c = 0; c < 3; ++c) z[k3 + c] = Mi[3 * c] * rr[0] + Mi[3 * c + 1] * rr[1] + Mi[3 * c + 2] * rr[2];
}
// p = z + beta p, q = S p (0 on inactive rows), beta = rz_new / rz
__global__ void k_pos_pcg_dir(uint32_t n_cams, const double* __restrict__ scal, int s_rzn, int s_rz, const uint8_t* __restrict__ active,
                              const double* __restrict__ S, const double* __restrict__ z, double* __restrict__ p, double* __restrict__ q) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double rz = scal[s_rz];
  const double beta = rz > 0.0 ? scal[s_rzn] / rz : 0.0;
  const size_t k3 = 3 * (size_t)k;
  for (int c = 0; c < 3; ++c) {
    const double pc = z[k3 + c] + beta * p[k3 + c];
    p[k3 + c] = pc;
    q[k3 + c] = active[k] ? S[k3 + c] * pc : 0.0;
  }
}

// The step in parameter space, delta = -S y (0 on inactive rows), and the scale-gauge direction v = x - x_fixed (0 on inactive rows; 0
// everywhere without a fixed camera or with the projection off)
__global__ void k_pos_step(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ S, const double* __restrict__ y,
                           const double* __restrict__ x, int32_t fixed, int gauge, double* __restrict__ delta, double* __restrict__ v) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t k3 = 3 * (size_t)k;
  for (int c = 0; c < 3; ++c) {
    delta[k3 + c] = active[k] ? -S[k3 + c] * y[k3 + c] : 0.0;
    v[k3 + c] = (active[k] && gauge && fixed >= 0) ? x[k3 + c] - x[3 * (size_t)fixed + c] : 0.0;
  }
}
// delta -= (delta.v / v.v) v (nothing when v = 0, e.g. at the all-zero start), cand = x + delta
__global__ void k_pos_project(uint32_t n_cams, const double* __restrict__ scal, int s_dv, int s_vv, const double* __restrict__ v,
                              double* __restrict__ delta, const double* __restrict__ x, double* __restrict__ cand) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double vv = scal[s_vv];
  const double beta = vv > 0.0 ? scal[s_dv] / vv : 0.0;
  const size_t k3 = 3 * (size_t)k;
  for (int c = 0; c < 3; ++c) {
    const double dc = delta[k3 + c] - beta * v[k3 + c];
    delta[k3 + c] = dc;
    cand[k3 + c] = x[k3 + c] + dc;
  }
}

// Exact step: the dense damped, scaled matrix S L S + D^2 in the tile layout of dense_kernels.hpp (lower triangle, right-hand side in
// block row T, identity on the padding).  One workgroup per camera row; inactive rows and columns are the identity.  Repeated pairs (two
// edges between the same cameras) are summed in CSR order by the thread of the run's first entry.
__global__ void __launch_bounds__(256) k_pos_dense_assemble(PosDev a, const double* __restrict__ S, const double* __restrict__ Mblk,
                                                            const double* __restrict__ b, double* __restrict__ A, uint32_t n, uint32_t T) {
  const uint32_t row = blockIdx.x;
  if (row >= a.n_cams) return;
  if (threadIdx.x == 0) {
    const double* M = Mblk + 6 * (size_t)row;
    const double m[9] = {M[0], M[1], M[2], M[1], M[3], M[4], M[2], M[4], M[5]};
    for (int r = 0; r < 3; ++r) for (int c = 0; c <= r; ++c) *dense_elem(A, 3 * row + r, 3 * row + c) = m[3 * r + c];
    for (int c = 0; c < 3; ++c) A[(((size_t)T * (T + 1) / 2) + (3 * row + c) / 32) * 1024 + (3 * row + c) % 32] = b[3 * (size_t)row + c];
    if (row == 0) for (uint32_t gg = n; gg < T * 32; ++gg) *dense_elem(A, gg, gg) = 1.0;
  }
  if (!a.active[row]) return;
  const uint32_t beg = a.row_ptr[row], end = a.row_ptr[row + 1];
  for (uint32_t d = beg + threadIdx.x; d < end; d += 256) {
    const uint32_t m = a.nbr[d];
    if (m >= row || !a.active[m] || (d > beg && a.nbr[d - 1] == m)) continue;
    double h[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t e = d; e < end && a.nbr[e] == m; ++e)
      for (int k = 0; k < 6; ++k) h[k] += a.H[6 * (size_t)e + k];
    const double H9[9] = {h[0], h[1], h[2], h[1], h[3], h[4], h[2], h[4], h[5]};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) *dense_elem(A, 3 * row + r, 3 * m + c) = -S[3 * (size_t)row + r] * H9[3 * r + c] * S[3 * (size_t)m + c];
  }
}

// d = R(aa)^T t with R = Ceres' AngleAxisToRotationMatrix (small-angle branch included): an edge's world direction from position_2 and
// the orientation of its first camera.  One routine for the position problem and for the translation filter (trans_filter_kernels.hpp).
__device__ __forceinline__ void pos_world_direction(const double* __restrict__ w, const double* __restrict__ t, double* d) {
  double R[9];
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 > DBL_EPSILON) {
    const double th = sqrt(th2), wx = w[0] / th, wy = w[1] / th, wz = w[2] / th, ct = cos(th), st = sin(th);
    R[0] = ct + wx * wx * (1.0 - ct); R[3] = wz * st + wx * wy * (1.0 - ct); R[6] = -wy * st + wx * wz * (1.0 - ct);
    R[1] = wx * wy * (1.0 - ct) - wz * st; R[4] = ct + wy * wy * (1.0 - ct); R[7] = wx * st + wy * wz * (1.0 - ct);
    R[2] = wy * st + wx * wz * (1.0 - ct); R[5] = -wx * st + wy * wz * (1.0 - ct); R[8] = ct + wz * wz * (1.0 - ct);
  } else {
    R[0] = 1.0; R[3] = w[2]; R[6] = -w[1];
    R[1] = -w[2]; R[4] = 1.0; R[7] = w[0];
    R[2] = w[1]; R[5] = -w[0]; R[8] = 1.0;
  }
  // (R is row-major here: R[3 r + c]); d = R^T t
  for (int c = 0; c < 3; ++c) d[c] = R[c] * t[0] + R[3 + c] * t[1] + R[6 + c] * t[2];
}

// world directions of the edges on the device, written for the edge and, with their signs, for its two directed entries
__global__ void k_pos_directions(uint32_t n_edges, const uint32_t* __restrict__ ei, const double* __restrict__ rot_aa, const double* __restrict__ rel_t,
                                 const uint32_t* __restrict__ pos_i, const uint32_t* __restrict__ pos_j, double* __restrict__ dir_e, double* __restrict__ dir_k) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  double d[3];
  pos_world_direction(rot_aa + 3 * (size_t)ei[e], rel_t + 3 * e, d);
  for (int c = 0; c < 3; ++c) { dir_e[3 * e + c] = d[c]; dir_k[3 * (size_t)pos_i[e] + c] = d[c]; dir_k[3 * (size_t)pos_j[e] + c] = -d[c]; }
}

}  // namespace gsfm
