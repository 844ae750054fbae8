// Device kernels of the full bundle adjustment (include/gsfm_ba6.h): camera orientations, camera positions and points move together.
//
// Structure.  With free orientations an observation's camera Jacobian is Jc = [Jr, -Jp] (2 x 6: the corrected Jacobians with respect to the
// angle-axis vector and, with J_pos = -J_point, to the centre), so the normal matrix has 6 x 6 camera blocks and 6 x 3 off-diagonal blocks
// and ba_kernels.hpp's block Laplacian is gone.  The products run MATRIX-FREE on the corrected Jacobians: per observation Jp (6 doubles) and
// Jr (6), 96 bytes per pass -- the stream of ba_kernels.hpp's H_e twice over, where the formed blocks Jc^T Jc, Jc^T Jp, Jp^T Jp would be 45
// doubles:  (J d)_e = Jr d_rot + Jp (d_point - d_pos).
//
// Unknowns are one array of (2 n_cams + n_tracks) x 3: the cameras' angle-axis vectors, the cameras' positions, the points -- three kinds
// of 3-vector nodes, so that the node-wise kernels of pos_kernels.hpp and ba_kernels.hpp (dots, reductions, Jacobi scale, D^2, the PCG
// direction) run unchanged; the points' inverses are this file's (k_ba6_prep_points: kept and applied in double-double).  `active` has one byte per node (a camera's two nodes carry the same byte), Dg holds the
// three 3 x 3 diagonal blocks per kind; the 3 x 3 block between a camera's two nodes goes to Bx (for gsfm_ba6_linearize, and for the last resort of k_ba6_cam_precond).
//
// Layout.  Per observation in the caller's (track-major) order: Jt (12 doubles: Jp rows 0 1, Jr rows 0 1) and Rt (2: r~), written by the
// POINT side of the linearisation, the only place that evaluates an observation.  The camera side copies Jt into its own order, Jc (one
// 96-byte gather per observation per linearisation), and reads Rt.  The camera records (k_ba6_cameras: R(w), f u v, the estimated flag and
// J_l(w), O(n_cams)) are rebuilt at every evaluation point, so that no observation pays for a sincos.
//
// Lane groups, row-per-wavefront, loop bounds, shuffles and the absence of atomics and of waits are those of ba_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ba_kernels.hpp"
#include "so3_dev.hpp"

namespace gsfm {

#define GSFM_BA6_CAM_DOUBLES 32   // R (9), unused (3), f u v, estimated (the record of k_tri_cameras), then J_l(w) (9) and padding to 256 bytes
#define GSFM_BA6_GAUGE 7          // translations (3), scale, rotations (3)
#define GSFM_BA6_GDOTS 35         // the upper triangle of V^T V (28, row-major) and V^T delta (7)

struct Ba6Dev {
  BaDev b;           // n_cams, n_tracks, the CSRs, track_used, active (2 N + T bytes), leaf; cams: GSFM_BA6_CAM_DOUBLES per camera; Ht, At, Hc unused
  double* Jt;        // n_obs x 12: Jp rows 0 1, Jr rows 0 1 in track order (zero for an unused observation)
  double* Rt;        // n_obs x 2: r~
  double* Jc;        // n_used x 12: Jt in camera order
};

__device__ __forceinline__ void ba6_load_j(const double* J, size_t i, double* j) {
  const double2* jp = (const double2*)(J + 12 * i);
#pragma unroll
  for (int k = 0; k < 6; ++k) { const double2 v = jp[k]; j[2 * k] = v.x; j[2 * k + 1] = v.y; }
}
__device__ __forceinline__ void ba6_store_j(double* J, size_t i, const double* j) {
  double2* jp = (double2*)(J + 12 * i);
#pragma unroll
  for (int k = 0; k < 6; ++k) jp[k] = make_double2(j[2 * k], j[2 * k + 1]);
}
// u = Jr a + Jp b (2-vector) for j = (Jp0, Jp1, Jr0, Jr1)
__device__ __forceinline__ void ba6_apply(const double* j, const double* a, const double* b, double& u0, double& u1) {
  u0 = j[6] * a[0] + j[7] * a[1] + j[8] * a[2] + j[0] * b[0] + j[1] * b[1] + j[2] * b[2];
  u1 = j[9] * a[0] + j[10] * a[1] + j[11] * a[2] + j[3] * b[0] + j[4] * b[1] + j[5] * b[2];
}

// The camera records at the evaluation point `at` (its first n_cams nodes are the angle-axis vectors).
__global__ void __launch_bounds__(256) k_ba6_cameras(uint32_t n_cams, const double* __restrict__ at, const double* __restrict__ intrinsics,
                                                     const uint8_t* __restrict__ cam_estimated, double* __restrict__ cams) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cams) return;
  const double w[3] = {at[3 * (size_t)c], at[3 * (size_t)c + 1], at[3 * (size_t)c + 2]};
  double R[9], T[9], Ti[9];
  rodrigues(w, R);
  jl_and_inverse(w, T, Ti);
  double* o = cams + (size_t)GSFM_BA6_CAM_DOUBLES * c;
#pragma unroll
  for (int k = 0; k < 9; ++k) { o[k] = R[k]; o[16 + k] = T[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[9 + k] = 0.0; o[12 + k] = intrinsics[3 * (size_t)c + k]; }
  o[15] = cam_estimated[c] ? 1.0 : 0.0;
#pragma unroll
  for (int k = 25; k < GSFM_BA6_CAM_DOUBLES; ++k) o[k] = 0.0;
}

// (the double-double pieces of the point solve -- ba6_two_sum .. ba6_apply_inv_dd, ba6_refine_inv3 -- are in ba_kernels.hpp, which uses them too)

// ---- point side ------------------------------------------------------------------------------------------------------------------
// Linearisation at x: per observation Jp, Jr and r~ (stored in track order), per point C_t = sum Jp^T Jp into Dg and g_t = sum Jp^T r~ into g.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba6_lin_tracks(Ba6Dev a6, BaSlots sl, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const BaDev& a = a6.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 2 * N + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_BA6_CAM_DOUBLES * c;
    double j[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r0 = 0.0, r1 = 0.0;
    if (used_t && cam[15] != 0.0) {
      double rho0;
      const double* o = x + 3 * (N + c);
      reproj_corrected6(cam, cam + 16, a.obs_xy[e], X[0] - o[0], X[1] - o[1], X[2] - o[2], a.leaf, j, j + 3, j + 6, j + 9, r0, r1, rho0);
      s[0] += j[0] * j[0] + j[3] * j[3]; s[1] += j[0] * j[1] + j[3] * j[4]; s[2] += j[0] * j[2] + j[3] * j[5];
      s[3] += j[1] * j[1] + j[4] * j[4]; s[4] += j[1] * j[2] + j[4] * j[5]; s[5] += j[2] * j[2] + j[5] * j[5];
      s[6] += j[0] * r0 + j[3] * r1; s[7] += j[1] * r0 + j[4] * r1; s[8] += j[2] * r0 + j[5] * r1;
    }
    ba6_store_j(a6.Jt, e, j);
    *(double2*)(a6.Rt + 2 * e) = make_double2(r0, r1);
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) s[q] = tri_group_allsum<G>(s[q]);
  if (tk.live && l == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Dg[6 * node + q] = s[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) g[3 * node + q] = s[6 + q];
  }
}

// Cost at x (the records hold R of x): cost_t[t] = sum over the track's used observations of rho(|r|^2) / 2.  r_out (n_obs x 2) and rho_out
// (n_obs), for gsfm_ba6_residuals, may be NULL; an unused observation gets zeros.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba6_cost_tracks(Ba6Dev a6, BaSlots sl, const double* __restrict__ x, double* __restrict__ cost_t,
                                                           double* __restrict__ r_out, double* __restrict__ rho_out) {
  const BaDev& a = a6.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 2 * N + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_BA6_CAM_DOUBLES * c;
    double ex = 0.0, ey = 0.0, rho = 0.0;
    if (used_t && cam[15] != 0.0) {
      const double* o = x + 3 * (N + c);
      reproj_residual(cam, a.obs_xy[e], X[0] - o[0], X[1] - o[1], X[2] - o[2], ex, ey);
      rho = loss_leaf_simple(a.leaf, ex * ex + ey * ey).r0;
      acc += 0.5 * rho;
    }
    if (r_out) { r_out[2 * e] = ex; r_out[2 * e + 1] = ey; }
    if (rho_out) rho_out[e] = rho;
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) cost_t[tk.t] = acc;
}

// The point pass of the Schur product and the back-substitution:  u_t = Cinv_t (sgn S_t sum_{e in t} Jp^T (Jc q_{k(e)}) + add_t), with q = S v
// on the cameras' nodes (0 on inactive ones), add = the node vector b or NULL.  scaled_out: out_t = S_t u_t (the z_t the camera pass
// gathers), else u_t.
//   Schur product      sgn = +1, add = NULL, scaled:  z = S C~^-1 E~^T v
//   back-substitution  sgn = -1, add = b:             y_p = C~^-1 (b_p - E~^T y_c)
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba6_point_pass(Ba6Dev a6, BaSlots sl, const double* __restrict__ q, const double* __restrict__ S,
                                                          const double* __restrict__ Cinv, const double* __restrict__ add, double sgn,
                                                          double* __restrict__ out, int scaled_out) {
  const BaDev& a = a6.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams;
  double yh[3] = {0.0, 0.0, 0.0}, yl[3] = {0.0, 0.0, 0.0};   // the track sums in double-double
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[12];
    ba6_load_j(a6.Jt, e, j);
    const double* qr = q + 3 * c, * qp = q + 3 * (N + c);
    // u = Jc q = Jr q_rot - Jp q_pos
    double uh[2] = {0.0, 0.0}, ul[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 3; ++i) { ba6_dd_mac(j[6 + 3 * r + i], qr[i], uh[r], ul[r]); ba6_dd_mac(-j[3 * r + i], qp[i], uh[r], ul[r]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) { ba6_dd_mac2(j[i], uh[0], ul[0], yh[i], yl[i]); ba6_dd_mac2(j[3 + i], uh[1], ul[1], yh[i], yl[i]); }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) ba6_group_allsum_dd<G>(yh[i], yl[i]);
  if (tk.live && l == 0) {
    const size_t node = 2 * N + tk.t;
    const double sc[3] = {S[3 * node], S[3 * node + 1], S[3 * node + 2]};
    double th[3], tl[3], u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // t = sgn S_t y + add_t, still a pair
      double hi = 0.0, lo = 0.0;
      ba6_dd_mac2(sgn * sc[i], yh[i], yl[i], hi, lo);
      if (add) ba6_dd_add(hi, lo, add[3 * node + i], 0.0);
      th[i] = hi; tl[i] = lo;
    }
    ba6_apply_inv_dd(Cinv + 18 * (size_t)tk.t, th, tl, u);
    double* o = out + 3 * (size_t)tk.t;
    o[0] = scaled_out ? sc[0] * u[0] : u[0]; o[1] = scaled_out ? sc[1] * u[1] : u[1]; o[2] = scaled_out ? sc[2] * u[2] : u[2];
  }
}

// quad_t[t] = sum_{e in t} |J~_e delta|^2 with J~_e delta = Jr d_rot + Jp (d_t - d_pos); jd_out (n_obs x 2, may be NULL) gets J~_e delta
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba6_quad_tracks(Ba6Dev a6, BaSlots sl, const double* __restrict__ delta, double* __restrict__ quad_t,
                                                           double* __restrict__ jd_out) {
  const BaDev& a = a6.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 2 * N + tk.t;
  double d[3] = {0.0, 0.0, 0.0};
  if (tk.live) { d[0] = delta[3 * node]; d[1] = delta[3 * node + 1]; d[2] = delta[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[12];
    ba6_load_j(a6.Jt, e, j);
    const double* dp = delta + 3 * (N + c);
    const double v[3] = {d[0] - dp[0], d[1] - dp[1], d[2] - dp[2]};
    double u0, u1;
    ba6_apply(j, delta + 3 * c, v, u0, u1);
    acc += u0 * u0 + u1 * u1;
    if (jd_out) { jd_out[2 * e] = u0; jd_out[2 * e + 1] = u1; }
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) quad_t[tk.t] = acc;
}

// ---- camera side: one wavefront per row -------------------------------------------------------------------------------------------
// The camera half of the linearisation: the row's Jacobians copied into camera order, g_rot = sum Jr^T r~, g_pos = -sum Jp^T r~, the diagonal
// blocks sum Jr^T Jr and sum Jp^T Jp into Dg and the block between the two, -sum Jr^T Jp (3 x 3, row-major), into Bx.
__global__ void __launch_bounds__(256) k_ba6_cam_lin(Ba6Dev a6, double* __restrict__ g, double* __restrict__ Dg, double* __restrict__ Bx) {
  const BaDev& a = a6.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  double acc[27];
#pragma unroll
  for (int q = 0; q < 27; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t e = a.cobs[d];
    double j[12];
    ba6_load_j(a6.Jt, e, j);
    ba6_store_j(a6.Jc, d, j);
    const double2 r = *(const double2*)(a6.Rt + 2 * e);
    const double* p0 = j, * p1 = j + 3, * q0 = j + 6, * q1 = j + 9;
#pragma unroll
    for (int c = 0; c < 3; ++c) { acc[c] += q0[c] * r.x + q1[c] * r.y; acc[3 + c] -= p0[c] * r.x + p1[c] * r.y; }
    acc[6] += q0[0] * q0[0] + q1[0] * q1[0]; acc[7] += q0[0] * q0[1] + q1[0] * q1[1]; acc[8] += q0[0] * q0[2] + q1[0] * q1[2];
    acc[9] += q0[1] * q0[1] + q1[1] * q1[1]; acc[10] += q0[1] * q0[2] + q1[1] * q1[2]; acc[11] += q0[2] * q0[2] + q1[2] * q1[2];
    acc[12] += p0[0] * p0[0] + p1[0] * p1[0]; acc[13] += p0[0] * p0[1] + p1[0] * p1[1]; acc[14] += p0[0] * p0[2] + p1[0] * p1[2];
    acc[15] += p0[1] * p0[1] + p1[1] * p1[1]; acc[16] += p0[1] * p0[2] + p1[1] * p1[2]; acc[17] += p0[2] * p0[2] + p1[2] * p1[2];
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[18 + 3 * r_ + c] -= q0[r_] * p0[c] + q1[r_] * p1[c];
  }
#pragma unroll
  for (int q = 0; q < 27; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    const size_t kr = row, kp = (size_t)a.n_cams + row;
    for (int c = 0; c < 3; ++c) { g[3 * kr + c] = acc[c]; g[3 * kp + c] = acc[3 + c]; }
    for (int c = 0; c < 6; ++c) { Dg[6 * kr + c] = acc[6 + c]; Dg[6 * kp + c] = acc[12 + c]; }
    for (int c = 0; c < 9; ++c) Bx[9 * kr + c] = acc[18 + c];
  }
}

// The camera pass:  out_k = S_k sum_{e in k} Jc^T (Jc q_k - Jp zs z_{t(e)}) + D2_k p_k + add_k  on active rows (q, p, add may be NULL: zero),
// written to the row's two nodes.  Inactive rows: p_k when identity_inactive (the PCG operator is the identity there), else 0.
//   Schur product   q = S p, z from the point pass, zs = 1:  out = Sc p
//   reduced rhs     q = NULL, z = -S C~^-1 b_p (k_ba6_prep_points), zs = -1, add = b:  out = b_c - E~ C~^-1 b_p
__global__ void __launch_bounds__(256) k_ba6_cam_pass(Ba6Dev a6, const double* __restrict__ q, const double* __restrict__ z, double zs,
                                                       const double* __restrict__ p, const double* __restrict__ S, const double* __restrict__ D2,
                                                       const double* __restrict__ add, double* __restrict__ out, int identity_inactive) {
  const BaDev& a = a6.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t r3 = 3 * (size_t)row, p3 = 3 * ((size_t)a.n_cams + row);
  if (!a.active[row]) {
    if (lane < 6) { const size_t i = lane < 3 ? r3 + lane : p3 + lane - 3; out[i] = (identity_inactive && p) ? p[i] : 0.0; }
    return;
  }
  double qr[3] = {0.0, 0.0, 0.0}, qp[3] = {0.0, 0.0, 0.0};
  if (q) { for (int c = 0; c < 3; ++c) { qr[c] = q[r3 + c]; qp[c] = q[p3 + c]; } }
  double y[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t t = a.ctrk[d];
    double j[12];
    ba6_load_j(a6.Jc, d, j);
    const double v[3] = {-(qp[0] + zs * z[3 * t]), -(qp[1] + zs * z[3 * t + 1]), -(qp[2] + zs * z[3 * t + 2])};
    double u0, u1;
    ba6_apply(j, qr, v, u0, u1);
#pragma unroll
    for (int c = 0; c < 3; ++c) { y[c] += j[6 + c] * u0 + j[9 + c] * u1; y[3 + c] -= j[c] * u0 + j[3 + c] * u1; }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) y[c] = wave_sum(y[c]);
  if (lane == 0) {
    for (int c = 0; c < 6; ++c) {
      const size_t i = c < 3 ? r3 + c : p3 + c - 3;
      double o = S[i] * y[c];
      if (p) o += D2[i] * p[i];
      if (add) o += add[i];
      out[i] = o;
    }
  }
}

// Cholesky M = L L^T of a symmetric positive definite 6 x 6 (full, row-major) and Minv = L^-T L^-1, in one lane.  false: a pivot was not
// positive (or not finite) -- M is not positive definite as computed and Minv is not to be used.
__device__ __forceinline__ bool ba6_inv6(const double* M, double* Minv) {
  double L[36], Li[36];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 36; ++i) { L[i] = 0.0; Li[i] = 0.0; }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double d = M[6 * c + c];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= L[6 * c + k] * L[6 * c + k];
    ok = ok && d > 0.0 && d <= DBL_MAX;
    const double l = sqrt(d);
    L[6 * c + c] = l;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double s = M[6 * r + c];
#pragma unroll
      for (int k = 0; k < c; ++k) s -= L[6 * r + k] * L[6 * c + k];
      L[6 * r + c] = s / l;
    }
  }
  // Li = L^-1 (lower triangular), column by column
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    Li[6 * c + c] = 1.0 / L[6 * c + c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) s -= L[6 * r + k] * Li[6 * k + c];
      Li[6 * r + c] = s / L[6 * r + r];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = r; k < 6; ++k) s += Li[6 * k + r] * Li[6 * k + c];
      Minv[6 * r + c] = s; Minv[6 * c + r] = s;
    }
  return ok;
}

// The preconditioner, the 6 x 6 block diagonal of the Schur complement (Ceres' SCHUR_JACOBI), inverted per camera:
//   M_k = S_k (sum_{e in k} Jc^T (I - Jp G_t Jp^T) Jc) S_k + D2_k,   G_t = S_t C~_t^-1 S_t;   the identity on inactive rows.
// G_t is plain fp64.  Where a point's block has lost rank (beyond the Tukey cut: one observation left) and is held up by the damping alone
// (1e-10 of its scaled diagonal at radius 1e10), Jp G_t Jp^T carries u cond(C~_t), W = I - Jp G_t Jp^T (of the damping's size) is noise and M_k
// can come out indefinite: its Cholesky fails.  Such a row is summed again with W from the pair inverse of k_ba6_prep_points, 1 - t^T C~^-1 t
// accumulated in double-double (t = S_t Jp^T); should that block fail too, the row takes the block of B~ alone, S_k B_k S_k + D2_k (Dg and Bx of
// k_ba6_cam_lin), positive definite by the damping.  Rows whose first Cholesky succeeds keep their bytes.  (Before, the NaNs of the failed
// factorisation made r.z NaN and the PCG returned y = 0 without a word.)
__device__ __forceinline__ void ba6_precond_add(const double* j, double w00, double w01, double w11, double* acc) {
  // the rows of Jc = [Jr, -Jp] and of W Jc
  double c0[6], c1[6], d0[6], d1[6];
#pragma unroll
  for (int c = 0; c < 3; ++c) { c0[c] = j[6 + c]; c1[c] = j[9 + c]; c0[3 + c] = -j[c]; c1[3 + c] = -j[3 + c]; }
#pragma unroll
  for (int c = 0; c < 6; ++c) { d0[c] = w00 * c0[c] + w01 * c1[c]; d1[c] = w01 * c0[c] + w11 * c1[c]; }
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) acc[q++] += c0[r] * d0[c] + c1[r] * d1[c];
}
__device__ __forceinline__ bool ba6_precond_invert(const double* acc, const double* s, const double* dd, double* M, double* inv) {
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { const double m = s[r] * acc[q++] * s[c] + (r == c ? dd[r] : 0.0); M[6 * r + c] = m; M[6 * c + r] = m; }
  return ba6_inv6(M, inv);
}
__global__ void __launch_bounds__(256) k_ba6_cam_precond(Ba6Dev a6, const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ Gt,
                                                          const double* __restrict__ Cinv, const double* __restrict__ Dg, const double* __restrict__ Bx,
                                                          double* __restrict__ Minv) {
  const BaDev& a = a6.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  double* Mi = Minv + 36 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 36) Mi[lane] = (lane % 7 == 0) ? 1.0 : 0.0;
    return;
  }
  double acc[21];
#pragma unroll
  for (int q = 0; q < 21; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[12], gt[6];
    ba6_load_j(a6.Jc, d, j);
    ba_load_h(Gt, a.ctrk[d], gt);
    // W = I - Jp G Jp^T (2 x 2, symmetric)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    ba_sym_mac(gt, j[0], j[1], j[2], a0, a1, a2);
    ba_sym_mac(gt, j[3], j[4], j[5], b0, b1, b2);
    const double w00 = 1.0 - (j[0] * a0 + j[1] * a1 + j[2] * a2), w01 = -(j[0] * b0 + j[1] * b1 + j[2] * b2), w11 = 1.0 - (j[3] * b0 + j[4] * b1 + j[5] * b2);
    ba6_precond_add(j, w00, w01, w11, acc);
  }
#pragma unroll
  for (int q = 0; q < 21; ++q) acc[q] = wave_sum(acc[q]);
  const size_t r3 = 3 * (size_t)row, p3 = 3 * ((size_t)a.n_cams + row);
  const double s[6] = {S[r3], S[r3 + 1], S[r3 + 2], S[p3], S[p3 + 1], S[p3 + 2]};
  const double dd[6] = {D2[r3], D2[r3 + 1], D2[r3 + 2], D2[p3], D2[p3 + 1], D2[p3 + 2]};
  int ok = 1;
  if (lane == 0) {
    double M[36], inv[36];
    ok = ba6_precond_invert(acc, s, dd, M, inv) ? 1 : 0;
    if (ok) for (int i = 0; i < 36; ++i) Mi[i] = inv[i];
  }
  if (__shfl(ok, 0, 64)) return;   // (wave-uniform)
  // the row again, W through the pair inverse
#pragma unroll
  for (int q = 0; q < 21; ++q) acc[q] = 0.0;
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[12];
    ba6_load_j(a6.Jc, d, j);
    const size_t t = a.ctrk[d], node = 2 * (size_t)a.n_cams + t;
    const double* Ci = Cinv + 18 * t;
    const double zl[3] = {0.0, 0.0, 0.0};
    double t0[3], t1[3], x0[3], x1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { t0[c] = S[3 * node + c] * j[c]; t1[c] = S[3 * node + c] * j[3 + c]; }
    ba6_apply_inv_dd(Ci, t0, zl, x0);
    ba6_apply_inv_dd(Ci, t1, zl, x1);
    double h00 = -1.0, l00 = 0.0, h01 = 0.0, l01 = 0.0, h11 = -1.0, l11 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ba6_dd_mac(t0[c], x0[c], h00, l00); ba6_dd_mac(t0[c], x1[c], h01, l01); ba6_dd_mac(t1[c], x1[c], h11, l11); }
    ba6_precond_add(j, -(h00 + l00), -(h01 + l01), -(h11 + l11), acc);
  }
#pragma unroll
  for (int q = 0; q < 21; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    double M[36], inv[36];
    if (!ba6_precond_invert(acc, s, dd, M, inv)) {
      // Last resort, reached by no test since the row is summed again above: B~'s block is positive definite by construction (a sum of
      // Jc^T Jc plus D2 > 0), so the result of its factorisation is not looked at; NaN inputs stay NaN and end as a stall in b6_pcg.
      const double* Dr = Dg + 6 * (size_t)row, * Dp = Dg + 6 * ((size_t)a.n_cams + row), * X = Bx + 9 * (size_t)row;
      const double Br[9] = {Dr[0], Dr[1], Dr[2], Dr[1], Dr[3], Dr[4], Dr[2], Dr[4], Dr[5]}, Bp[9] = {Dp[0], Dp[1], Dp[2], Dp[1], Dp[3], Dp[4], Dp[2], Dp[4], Dp[5]};
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          M[6 * r + c] = s[r] * Br[3 * r + c] * s[c] + (r == c ? dd[r] : 0.0);
          M[6 * (3 + r) + 3 + c] = s[3 + r] * Bp[3 * r + c] * s[3 + c] + (r == c ? dd[3 + r] : 0.0);
          M[6 * r + 3 + c] = M[6 * (3 + c) + r] = s[r] * X[3 * r + c] * s[3 + c];
        }
      ba6_inv6(M, inv);
    }
    for (int i = 0; i < 36; ++i) Mi[i] = inv[i];
  }
}

// ---- the points' inverses ------------------------------------------------------------------------------------------------------------
// k_ba_prep_points with the inverse as a pair: C~_t = S_t C_t S_t + D2_t inverted by cofactors, two Newton steps and the third step's
// correction kept beside it (Cinv: 18 doubles per point); zneg through the pair, G_t (the preconditioner's) from its first half.
__global__ void k_ba6_prep_points(uint32_t n_cam_nodes, uint32_t n_tracks, const uint8_t* __restrict__ active, const double* __restrict__ Dg,
                                  const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ b, double* __restrict__ Cinv,
                                  double* __restrict__ Gt, double* __restrict__ zneg) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tracks) return;
  const size_t node = (size_t)n_cam_nodes + t;
  double Ci[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, G6[6] = {0, 0, 0, 0, 0, 0}, zn[3] = {0, 0, 0};
  if (active[node]) {
    const double* D = Dg + 6 * node;
    const double s0 = S[3 * node], s1 = S[3 * node + 1], s2 = S[3 * node + 2];
    const double M[6] = {s0 * D[0] * s0 + D2[3 * node], s0 * D[1] * s1, s0 * D[2] * s2, s1 * D[3] * s1 + D2[3 * node + 1], s1 * D[4] * s2,
                         s2 * D[5] * s2 + D2[3 * node + 2]};
    pos_inv3(M, Ci);
    ba6_refine_inv3(M, Ci, nullptr);
    ba6_refine_inv3(M, Ci, nullptr);
    ba6_refine_inv3(M, Ci, Ci + 9);   // the third step's correction is kept beside X: C~^-1 = Ci[0..8] + Ci[9..17] to about u^2
    G6[0] = s0 * Ci[0] * s0; G6[1] = s0 * Ci[1] * s1; G6[2] = s0 * Ci[2] * s2; G6[3] = s1 * Ci[4] * s1; G6[4] = s1 * Ci[5] * s2; G6[5] = s2 * Ci[8] * s2;
    const double bh[3] = {b[3 * node], b[3 * node + 1], b[3 * node + 2]}, bl[3] = {0.0, 0.0, 0.0};
    double w[3];
    ba6_apply_inv_dd(Ci, bh, bl, w);
    zn[0] = -s0 * w[0]; zn[1] = -s1 * w[1]; zn[2] = -s2 * w[2];
  }
  for (int c = 0; c < 18; ++c) Cinv[18 * t + c] = Ci[c];
  for (int c = 0; c < 6; ++c) Gt[6 * t + c] = G6[c];
  for (int c = 0; c < 3; ++c) zneg[3 * t + c] = zn[c];
}

// ---- PCG on the cameras' 6-vectors (the two nodes of a camera) ------------------------------------------------------------------------
__device__ __forceinline__ void ba6_apply_minv(const double* Mi, const double* r, double* z) {
#pragma unroll
  for (int c = 0; c < 6; ++c) z[c] = Mi[6 * c] * r[0] + Mi[6 * c + 1] * r[1] + Mi[6 * c + 2] * r[2] + Mi[6 * c + 3] * r[3] + Mi[6 * c + 4] * r[4] + Mi[6 * c + 5] * r[5];
}
// PCG start: y = 0, r = rhs, z = M^-1 r, p = z, q = S p (0 on inactive rows)
__global__ void k_ba6_pcg_init(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ rhs, const double* __restrict__ Minv,
                               const double* __restrict__ S, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                               double* __restrict__ q) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t r3 = 3 * (size_t)k, p3 = 3 * ((size_t)n_cams + k);
  double rr[6], zz[6];
  for (int c = 0; c < 6; ++c) rr[c] = rhs[c < 3 ? r3 + c : p3 + c - 3];
  ba6_apply_minv(Minv + 36 * (size_t)k, rr, zz);
  for (int c = 0; c < 6; ++c) {
    const size_t i = c < 3 ? r3 + c : p3 + c - 3;
    y[i] = 0.0; r[i] = rr[c]; z[i] = zz[c]; p[i] = zz[c];
    q[i] = active[k] ? S[i] * zz[c] : 0.0;
  }
}
// y += alpha p, r -= alpha A p, z = M^-1 r with alpha = rz / pAp from the device scalars (k_pos_pcg_update with 6 x 6 blocks)
__global__ void k_ba6_pcg_update(uint32_t n_cams, const double* __restrict__ scal, int s_rz, int s_pap, const double* __restrict__ p,
                                 const double* __restrict__ Ap, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z,
                                 const double* __restrict__ Minv) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double pap = scal[s_pap];
  const double alpha = pap > 0.0 ? scal[s_rz] / pap : 0.0;
  const size_t r3 = 3 * (size_t)k, p3 = 3 * ((size_t)n_cams + k);
  double rr[6], zz[6];
  for (int c = 0; c < 6; ++c) {
    const size_t i = c < 3 ? r3 + c : p3 + c - 3;
    y[i] += alpha * p[i]; rr[c] = r[i] - alpha * Ap[i]; r[i] = rr[c];
  }
  ba6_apply_minv(Minv + 36 * (size_t)k, rr, zz);
  for (int c = 0; c < 6; ++c) z[c < 3 ? r3 + c : p3 + c - 3] = zz[c];
}

// ---- the gauge ---------------------------------------------------------------------------------------------------------------------
// The seven null directions of J at x on one node (gsfm_ba6.h): translations e_c, scaling x - mean, rotations (e_c x x on a centre or a
// point, -J_l(w)^-T e_c = minus row c of J_l(w)^-1 on an orientation).  kind 0: an orientation node, else a centre or a point.
__device__ __forceinline__ void ba6_gauge_dirs(int kind, const double* xn, const double* mean, double v[GSFM_BA6_GAUGE][3]) {
#pragma unroll
  for (int i = 0; i < GSFM_BA6_GAUGE; ++i) { v[i][0] = 0.0; v[i][1] = 0.0; v[i][2] = 0.0; }
  if (kind == 0) {
    double T[9], Ti[9];
    jl_and_inverse(xn, T, Ti);
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[4 + c][0] = -Ti[3 * c]; v[4 + c][1] = -Ti[3 * c + 1]; v[4 + c][2] = -Ti[3 * c + 2]; }
  } else {
    v[0][0] = 1.0; v[1][1] = 1.0; v[2][2] = 1.0;
    v[3][0] = xn[0] - mean[0]; v[3][1] = xn[1] - mean[1]; v[3][2] = xn[2] - mean[2];
    v[4][1] = -xn[2]; v[4][2] = xn[1];    // e_x x X
    v[5][0] = xn[2]; v[5][2] = -xn[0];    // e_y x X
    v[6][0] = -xn[1]; v[6][1] = xn[0];    // e_z x X
  }
}
// part[i * GSFM_POS_PARTS + block]: the block's share of the 35 dots (the upper triangle of V^T V, then V^T delta) over the active nodes;
// scal[s_x .. s_x + 2] the axis sums of x over the active centres and points, inv_count = 1 / their number
__global__ void __launch_bounds__(256) k_ba6_gauge_dots(uint32_t n_cams, size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ x,
                                                         const double* __restrict__ delta, const double* __restrict__ scal, int s_x, double inv_count,
                                                         double* __restrict__ part) {
  __shared__ double lds[5];
  const double mean[3] = {scal[s_x] * inv_count, scal[s_x + 1] * inv_count, scal[s_x + 2] * inv_count};
  double acc[GSFM_BA6_GDOTS];
#pragma unroll
  for (int i = 0; i < GSFM_BA6_GDOTS; ++i) acc[i] = 0.0;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n_nodes; k += (size_t)GSFM_POS_PARTS * 256) {
    if (!active[k]) continue;
    double v[GSFM_BA6_GAUGE][3];
    ba6_gauge_dirs(k < n_cams ? 0 : 1, x + 3 * k, mean, v);
    const double d0 = delta[3 * k], d1 = delta[3 * k + 1], d2 = delta[3 * k + 2];
    int q = 0;
#pragma unroll
    for (int i = 0; i < GSFM_BA6_GAUGE; ++i)
#pragma unroll
      for (int j = i; j < GSFM_BA6_GAUGE; ++j) acc[q++] += v[i][0] * v[j][0] + v[i][1] * v[j][1] + v[i][2] * v[j][2];
#pragma unroll
    for (int i = 0; i < GSFM_BA6_GAUGE; ++i) acc[28 + i] += v[i][0] * d0 + v[i][1] * d1 + v[i][2] * d2;
  }
#pragma unroll
  for (int i = 0; i < GSFM_BA6_GDOTS; ++i) {
    const double t = block_sum_bcast(acc[i], lds);
    if (threadIdx.x == 0) part[(size_t)i * GSFM_POS_PARTS + blockIdx.x] = t;
  }
}
// out[i] = the sum of dot i's partials, in the order of k_pos_reduce; one workgroup per dot
__global__ void __launch_bounds__(256) k_ba6_gauge_reduce(const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (int k = threadIdx.x; k < GSFM_POS_PARTS; k += 256) acc += part[(size_t)blockIdx.x * GSFM_POS_PARTS + k];
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}
// delta -= V c on the active nodes (c = scal[s_c .. s_c + 6]; all zero without the projection), cand = x + delta
__global__ void k_ba6_gauge_apply(uint32_t n_cams, size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ x,
                                  const double* __restrict__ scal, int s_x, double inv_count, int s_c, int project, double* __restrict__ delta,
                                  double* __restrict__ cand) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_nodes) return;
  double d[3] = {delta[3 * k], delta[3 * k + 1], delta[3 * k + 2]};
  if (project && active[k]) {
    const double mean[3] = {scal[s_x] * inv_count, scal[s_x + 1] * inv_count, scal[s_x + 2] * inv_count};
    double v[GSFM_BA6_GAUGE][3];
    ba6_gauge_dirs(k < n_cams ? 0 : 1, x + 3 * k, mean, v);
#pragma unroll
    for (int i = 0; i < GSFM_BA6_GAUGE; ++i) {
      const double c = scal[s_c + i];
      d[0] -= c * v[i][0]; d[1] -= c * v[i][1]; d[2] -= c * v[i][2];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { delta[3 * k + c] = d[c]; cand[3 * k + c] = x[3 * k + c] + d[c]; }
}

}  // namespace gsfm
