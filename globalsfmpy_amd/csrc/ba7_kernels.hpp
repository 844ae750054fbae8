// Device kernels of the full bundle adjustment with free focal lengths (include/gsfm_ba7.h): the counterparts of ba6_kernels.hpp with a
// seventh coordinate per camera.
//
// Structure.  An observation's camera Jacobian is Jc = [Jr, -Jp, Jf] (2 x 7), the normal matrix has 7 x 7 camera blocks and 7 x 3
// off-diagonal blocks, and the products run matrix-free on the corrected Jacobians as in ba6_kernels.hpp: per observation Jp (6 doubles),
// Jr (6) and Jf (2), seven 16-byte pieces, 112 bytes per pass:  (J d)_e = Jr d_rot + Jp (d_point - d_pos) + Jf d_f.
//
// Unknowns are one array of (3 n_cams + n_tracks) x 3: the cameras' angle-axis vectors, the cameras' centres, the cameras' INTRINSICS NODES
// (f, 0, 0), the points -- four kinds of 3-vector nodes, so that the node-wise kernels of pos_kernels.hpp and ba_kernels.hpp (dots, norms,
// reductions, Jacobi scale, D^2, the PCG direction, k_ba_scale) and k_ba6_prep_points run unchanged.  (The two spare coordinates leave room
// for k1 k2.)  `active` has one byte per node: a camera's first two nodes carry the camera's byte, its intrinsics node carries
// `camera active && focal_free`; a held focal length is thereby no parameter: it enters no norm, gets a zero step from k_ba_scale and a zero q
// from k_pos_pcg_dir, and the kernels below read its value from x like any other.
// INVARIANT: the two padding coordinates of an intrinsics node are exact zeros (+0 or -0) in every vector that a dot, a norm or the gauge
// sums read: x, cand, g, b, y, delta, rhs, r, z, p, q, Ap.  x gets them from the upload; every kernel here that writes one of the others
// writes the zeros itself (k_ba7_cam_lin: g and Dg; k_ba7_cam_pass: rhs and Ap; k_ba7_pcg_init / k_ba7_pcg_update: y, r, z, p, q); the
// node-wise kernels keep them (S = 1 and D^2 = min_lm_diagonal / radius there multiply zeros only).  The same holds for the focal
// coordinate of a camera whose focal length is held.
// Dg holds the 3 x 3 diagonal blocks per node, (B_ff, 0, 0, 0, 0, 0) on an intrinsics node; the blocks between a camera's nodes go to Bx,
// GSFM_BA7_BX doubles per camera: w x o (9, row-major), w x f (3), o x f (3), one spare.
//
// Layout per observation, lane groups, row-per-wavefront, loop bounds, shuffles and the absence of atomics and of waits are those of
// ba6_kernels.hpp; the camera record is its record with f taken from the evaluation point, not from `intrinsics`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ba6_kernels.hpp"

namespace gsfm {

#define GSFM_BA7_J 14    // Jp rows 0 1 (6), Jr rows 0 1 (6), Jf (2)
#define GSFM_BA7_BX 16
#define GSFM_BA7_TRI 28  // the upper triangle of a 7 x 7, row-major

struct Ba7Dev {
  BaDev b;           // as Ba6Dev's; active: 3 N + T bytes
  double* Jt;        // n_obs x 14 in track order (zero for an unused observation)
  double* Rt;        // n_obs x 2: r~
  double* Jc;        // n_used x 14: Jt in camera order
};

__device__ __forceinline__ void ba7_load_j(const double* J, size_t i, double* j) {
  const double2* jp = (const double2*)(J + GSFM_BA7_J * i);
#pragma unroll
  for (int k = 0; k < 7; ++k) { const double2 v = jp[k]; j[2 * k] = v.x; j[2 * k + 1] = v.y; }
}
__device__ __forceinline__ void ba7_store_j(double* J, size_t i, const double* j) {
  double2* jp = (double2*)(J + GSFM_BA7_J * i);
#pragma unroll
  for (int k = 0; k < 7; ++k) jp[k] = make_double2(j[2 * k], j[2 * k + 1]);
}
// the rows of Jc = [Jr, -Jp, Jf] for j = (Jp0, Jp1, Jr0, Jr1, Jf)
__device__ __forceinline__ void ba7_rows(const double* j, double* c0, double* c1) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { c0[c] = j[6 + c]; c1[c] = j[9 + c]; c0[3 + c] = -j[c]; c1[3 + c] = -j[3 + c]; }
  c0[6] = j[12]; c1[6] = j[13];
}
// the index of coordinate c (w, o, f) of camera `row` in a node vector
__device__ __forceinline__ size_t ba7_at(size_t n_cams, size_t row, int c) {
  return c < 3 ? 3 * row + c : c < 6 ? 3 * (n_cams + row) + c - 3 : 3 * (2 * n_cams + row);
}
__device__ __forceinline__ constexpr int ba7_tri(int r, int c) { return r * 7 - r * (r - 1) / 2 + (c - r); }   // r <= c

// The camera records at the evaluation point `at`: k_ba6_cameras' record with f from the camera's intrinsics node.
__global__ void __launch_bounds__(256) k_ba7_cameras(uint32_t n_cams, const double* __restrict__ at, const double* __restrict__ intrinsics,
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
  for (int k = 0; k < 3; ++k) o[9 + k] = 0.0;
  o[12] = at[3 * (2 * (size_t)n_cams + c)];
  o[13] = intrinsics[3 * (size_t)c + 1]; o[14] = intrinsics[3 * (size_t)c + 2];
  o[15] = cam_estimated[c] ? 1.0 : 0.0;
#pragma unroll
  for (int k = 25; k < GSFM_BA6_CAM_DOUBLES; ++k) o[k] = 0.0;
}

// ---- point side ------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba7_lin_tracks(Ba7Dev a7, BaSlots sl, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const BaDev& a = a7.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 3 * N + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_BA6_CAM_DOUBLES * c;
    double j[GSFM_BA7_J] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r0 = 0.0, r1 = 0.0;
    if (used_t && cam[15] != 0.0) {
      double rho0;
      const double* o = x + 3 * (N + c);
      reproj_corrected7(cam, cam + 16, a.obs_xy[e], X[0] - o[0], X[1] - o[1], X[2] - o[2], a.leaf, j, j + 3, j + 6, j + 9, j + 12, r0, r1, rho0);
      s[0] += j[0] * j[0] + j[3] * j[3]; s[1] += j[0] * j[1] + j[3] * j[4]; s[2] += j[0] * j[2] + j[3] * j[5];
      s[3] += j[1] * j[1] + j[4] * j[4]; s[4] += j[1] * j[2] + j[4] * j[5]; s[5] += j[2] * j[2] + j[5] * j[5];
      s[6] += j[0] * r0 + j[3] * r1; s[7] += j[1] * r0 + j[4] * r1; s[8] += j[2] * r0 + j[5] * r1;
    }
    ba7_store_j(a7.Jt, e, j);
    *(double2*)(a7.Rt + 2 * e) = make_double2(r0, r1);
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

// Cost at x (the records hold R and f of x); r_out / rho_out as k_ba6_cost_tracks
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba7_cost_tracks(Ba7Dev a7, BaSlots sl, const double* __restrict__ x, double* __restrict__ cost_t,
                                                           double* __restrict__ r_out, double* __restrict__ rho_out) {
  const BaDev& a = a7.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 3 * N + tk.t;
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

// The point pass of the Schur product and the back-substitution, as k_ba6_point_pass:  u = Jc q = Jr q_rot - Jp q_pos + Jf q_f  (q is 0 on an
// inactive node, a held focal length's included).
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba7_point_pass(Ba7Dev a7, BaSlots sl, const double* __restrict__ q, const double* __restrict__ S,
                                                          const double* __restrict__ Cinv, const double* __restrict__ add, double sgn,
                                                          double* __restrict__ out, int scaled_out) {
  const BaDev& a = a7.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams;
  double yh[3] = {0.0, 0.0, 0.0}, yl[3] = {0.0, 0.0, 0.0};   // the track sums in double-double
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[GSFM_BA7_J];
    ba7_load_j(a7.Jt, e, j);
    const double* qr = q + 3 * c, * qp = q + 3 * (N + c);
    const double qf = q[3 * (2 * N + c)];
    double uh[2] = {0.0, 0.0}, ul[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { ba6_dd_mac(j[6 + 3 * r + i], qr[i], uh[r], ul[r]); ba6_dd_mac(-j[3 * r + i], qp[i], uh[r], ul[r]); }
      ba6_dd_mac(j[12 + r], qf, uh[r], ul[r]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { ba6_dd_mac2(j[i], uh[0], ul[0], yh[i], yl[i]); ba6_dd_mac2(j[3 + i], uh[1], ul[1], yh[i], yl[i]); }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) ba6_group_allsum_dd<G>(yh[i], yl[i]);
  if (tk.live && l == 0) {
    const size_t node = 3 * N + tk.t;
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

// quad_t[t] = sum_{e in t} |J~_e delta|^2 with J~_e delta = Jr d_rot + Jp (d_t - d_pos) + Jf d_f; jd_out (n_obs x 2, may be NULL) gets J~_e delta
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba7_quad_tracks(Ba7Dev a7, BaSlots sl, const double* __restrict__ delta, double* __restrict__ quad_t,
                                                           double* __restrict__ jd_out) {
  const BaDev& a = a7.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = 3 * N + tk.t;
  double d[3] = {0.0, 0.0, 0.0};
  if (tk.live) { d[0] = delta[3 * node]; d[1] = delta[3 * node + 1]; d[2] = delta[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[GSFM_BA7_J];
    ba7_load_j(a7.Jt, e, j);
    const double* dp = delta + 3 * (N + c);
    const double v[3] = {d[0] - dp[0], d[1] - dp[1], d[2] - dp[2]};
    const double df = delta[3 * (2 * N + c)];
    double u0, u1;
    ba6_apply(j, delta + 3 * c, v, u0, u1);
    u0 += j[12] * df; u1 += j[13] * df;
    acc += u0 * u0 + u1 * u1;
    if (jd_out) { jd_out[2 * e] = u0; jd_out[2 * e + 1] = u1; }
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) quad_t[tk.t] = acc;
}

// ---- camera side: one wavefront per row -------------------------------------------------------------------------------------------
// The camera half of the linearisation: the row's Jacobians copied into camera order, g_k = sum Jc^T r~ (7) and B_k = sum Jc^T Jc (the 28
// entries of its upper triangle), scattered to g, Dg and Bx.  A held focal length gets zeros in its entry, row and column.
__global__ void __launch_bounds__(256) k_ba7_cam_lin(Ba7Dev a7, double* __restrict__ g, double* __restrict__ Dg, double* __restrict__ Bx) {
  const BaDev& a = a7.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  double acc[7 + GSFM_BA7_TRI];
#pragma unroll
  for (int q = 0; q < 7 + GSFM_BA7_TRI; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t e = a.cobs[d];
    double j[GSFM_BA7_J], c0[7], c1[7];
    ba7_load_j(a7.Jt, e, j);
    ba7_store_j(a7.Jc, d, j);
    const double2 r = *(const double2*)(a7.Rt + 2 * e);
    ba7_rows(j, c0, c1);
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] += c0[c] * r.x + c1[c] * r.y;
    int q = 7;
#pragma unroll
    for (int rr = 0; rr < 7; ++rr)
#pragma unroll
      for (int c = rr; c < 7; ++c) acc[q++] += c0[rr] * c0[c] + c1[rr] * c1[c];
  }
#pragma unroll
  for (int q = 0; q < 7 + GSFM_BA7_TRI; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    const size_t N = a.n_cams, kr = row, kp = N + row, kf = 2 * N + row;
    const double ff = a.active[kf] ? 1.0 : 0.0;   // (a held focal length: exact zeros)
    const double* B = acc + 7;
    for (int c = 0; c < 3; ++c) { g[3 * kr + c] = acc[c]; g[3 * kp + c] = acc[3 + c]; }
    g[3 * kf] = ff * acc[6]; g[3 * kf + 1] = 0.0; g[3 * kf + 2] = 0.0;
    int q = 0;
    for (int r = 0; r < 3; ++r)
      for (int c = r; c < 3; ++c) { Dg[6 * kr + q] = B[ba7_tri(r, c)]; Dg[6 * kp + q] = B[ba7_tri(3 + r, 3 + c)]; ++q; }
    Dg[6 * kf] = ff * B[ba7_tri(6, 6)];
    for (int c = 1; c < 6; ++c) Dg[6 * kf + c] = 0.0;
    double* X = Bx + GSFM_BA7_BX * (size_t)row;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) X[3 * r + c] = B[ba7_tri(r, 3 + c)];
      X[9 + r] = ff * B[ba7_tri(r, 6)]; X[12 + r] = ff * B[ba7_tri(3 + r, 6)];
    }
    X[15] = 0.0;
  }
}

// The camera pass, as k_ba6_cam_pass over 7 coordinates:  out_k = S_k sum_{e in k} Jc^T (Jc q_k - Jp zs z_{t(e)}) + D2_k p_k + add_k.  On an
// inactive row and on a held focal coordinate: p when identity_inactive, else 0.  The padding of the intrinsics node gets zeros.
__global__ void __launch_bounds__(256) k_ba7_cam_pass(Ba7Dev a7, const double* __restrict__ q, const double* __restrict__ z, double zs,
                                                       const double* __restrict__ p, const double* __restrict__ S, const double* __restrict__ D2,
                                                       const double* __restrict__ add, double* __restrict__ out, int identity_inactive) {
  const BaDev& a = a7.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t N = a.n_cams, f3 = 3 * (2 * N + row);
  if (!a.active[row]) {
    if (lane < 7) { const size_t i = ba7_at(N, row, lane); out[i] = (identity_inactive && p) ? p[i] : 0.0; }
    if (lane == 0) { out[f3 + 1] = 0.0; out[f3 + 2] = 0.0; }
    return;
  }
  double qq[7] = {0, 0, 0, 0, 0, 0, 0};
  if (q) {
#pragma unroll
    for (int c = 0; c < 7; ++c) qq[c] = q[ba7_at(N, row, c)];
  }
  double y[7] = {0, 0, 0, 0, 0, 0, 0};
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t t = a.ctrk[d];
    double j[GSFM_BA7_J], c0[7], c1[7];
    ba7_load_j(a7.Jc, d, j);
    ba7_rows(j, c0, c1);
    const double v[3] = {-(qq[3] + zs * z[3 * t]), -(qq[4] + zs * z[3 * t + 1]), -(qq[5] + zs * z[3 * t + 2])};
    double u0, u1;
    ba6_apply(j, qq, v, u0, u1);
    u0 += j[12] * qq[6]; u1 += j[13] * qq[6];
#pragma unroll
    for (int c = 0; c < 7; ++c) y[c] += c0[c] * u0 + c1[c] * u1;
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) y[c] = wave_sum(y[c]);
  if (lane == 0) {
    const bool ff = a.active[2 * N + row] != 0;
    for (int c = 0; c < 7; ++c) {
      const size_t i = ba7_at(N, row, c);
      double o = S[i] * y[c];
      if (p) o += D2[i] * p[i];
      if (add) o += add[i];
      if (c == 6 && !ff) o = (identity_inactive && p) ? p[i] : 0.0;
      out[i] = o;
    }
    out[f3 + 1] = 0.0; out[f3 + 2] = 0.0;
  }
}

// Cholesky M = L L^T of a symmetric positive definite 7 x 7 (full, row-major) and Minv = L^-T L^-1, in one lane (ba6_inv6 at order 7).
__device__ __forceinline__ bool ba7_inv7(const double* M, double* Minv) {
  constexpr int D = 7;
  double L[D * D], Li[D * D];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < D * D; ++i) { L[i] = 0.0; Li[i] = 0.0; }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    double d = M[D * c + c];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= L[D * c + k] * L[D * c + k];
    ok = ok && d > 0.0 && d <= DBL_MAX;
    const double l = sqrt(d);
    L[D * c + c] = l;
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      double s = M[D * r + c];
#pragma unroll
      for (int k = 0; k < c; ++k) s -= L[D * r + k] * L[D * c + k];
      L[D * r + c] = s / l;
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    Li[D * c + c] = 1.0 / L[D * c + c];
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) s -= L[D * r + k] * Li[D * k + c];
      Li[D * r + c] = s / L[D * r + r];
    }
  }
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = r; k < D; ++k) s += Li[D * k + r] * Li[D * k + c];
      Minv[D * r + c] = s; Minv[D * c + r] = s;
    }
  return ok;
}

// The preconditioner, the 7 x 7 block diagonal of the Schur complement inverted per camera, with k_ba6_cam_precond's three tiers: W = I - Jp
// G_t Jp^T in plain fp64; for a row whose block that leaves indefinite, W through the pair inverse; should that fail too, the block of B~
// alone.  A held focal coordinate is decoupled (zero row and column, diagonal 1): the other six get ba6's numbers.  The identity on inactive rows.
__device__ __forceinline__ void ba7_precond_add(const double* j, double w00, double w01, double w11, double* acc) {
  double c0[7], c1[7], d0[7], d1[7];
  ba7_rows(j, c0, c1);
#pragma unroll
  for (int c = 0; c < 7; ++c) { d0[c] = w00 * c0[c] + w01 * c1[c]; d1[c] = w01 * c0[c] + w11 * c1[c]; }
  int q = 0;
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = r; c < 7; ++c) acc[q++] += c0[r] * d0[c] + c1[r] * d1[c];
}
// M = S acc S + D2 from the 28 sums (focal_free = false: the focal coordinate decoupled), inverted
__device__ __forceinline__ bool ba7_precond_invert(const double* acc, const double* s, const double* dd, bool focal_free, double* M, double* inv) {
  int q = 0;
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = r; c < 7; ++c) {
      double m = s[r] * acc[q++] * s[c] + (r == c ? dd[r] : 0.0);
      if (c == 6 && !focal_free) m = r == 6 ? 1.0 : 0.0;
      M[7 * r + c] = m; M[7 * c + r] = m;
    }
  return ba7_inv7(M, inv);
}
__global__ void __launch_bounds__(256) k_ba7_cam_precond(Ba7Dev a7, const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ Gt,
                                                          const double* __restrict__ Cinv, const double* __restrict__ Dg, const double* __restrict__ Bx,
                                                          double* __restrict__ Minv) {
  const BaDev& a = a7.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  double* Mi = Minv + 49 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 49) Mi[lane] = (lane % 8 == 0) ? 1.0 : 0.0;
    return;
  }
  const size_t N = a.n_cams;
  const bool ff = a.active[2 * N + row] != 0;
  double acc[GSFM_BA7_TRI];
#pragma unroll
  for (int q = 0; q < GSFM_BA7_TRI; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[GSFM_BA7_J], gt[6];
    ba7_load_j(a7.Jc, d, j);
    ba_load_h(Gt, a.ctrk[d], gt);
    // W = I - Jp G Jp^T (2 x 2, symmetric)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    ba_sym_mac(gt, j[0], j[1], j[2], a0, a1, a2);
    ba_sym_mac(gt, j[3], j[4], j[5], b0, b1, b2);
    const double w00 = 1.0 - (j[0] * a0 + j[1] * a1 + j[2] * a2), w01 = -(j[0] * b0 + j[1] * b1 + j[2] * b2), w11 = 1.0 - (j[3] * b0 + j[4] * b1 + j[5] * b2);
    ba7_precond_add(j, w00, w01, w11, acc);
  }
#pragma unroll
  for (int q = 0; q < GSFM_BA7_TRI; ++q) acc[q] = wave_sum(acc[q]);
  double s[7], dd[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) { const size_t i = ba7_at(N, row, c); s[c] = S[i]; dd[c] = D2[i]; }
  int ok = 1;
  if (lane == 0) {
    double M[49], inv[49];
    ok = ba7_precond_invert(acc, s, dd, ff, M, inv) ? 1 : 0;
    if (ok) for (int i = 0; i < 49; ++i) Mi[i] = inv[i];
  }
  if (__shfl(ok, 0, 64)) return;   // (wave-uniform)
  // the row again, W through the pair inverse
#pragma unroll
  for (int q = 0; q < GSFM_BA7_TRI; ++q) acc[q] = 0.0;
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[GSFM_BA7_J];
    ba7_load_j(a7.Jc, d, j);
    const size_t t = a.ctrk[d], node = 3 * N + t;
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
    ba7_precond_add(j, -(h00 + l00), -(h01 + l01), -(h11 + l11), acc);
  }
#pragma unroll
  for (int q = 0; q < GSFM_BA7_TRI; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    double M[49], inv[49];
    if (!ba7_precond_invert(acc, s, dd, ff, M, inv)) {
      // Last resort, as k_ba6_cam_precond's: B~'s block, S_k B_k S_k + D2_k from Dg and Bx (a held focal length has zeros there already)
      const double* Dr = Dg + 6 * (size_t)row, * Dp = Dg + 6 * (N + row), * X = Bx + GSFM_BA7_BX * (size_t)row;
      double B[GSFM_BA7_TRI];
      int q = 0;
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) { B[ba7_tri(r, c)] = Dr[q]; B[ba7_tri(3 + r, 3 + c)] = Dp[q]; ++q; }
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) B[ba7_tri(r, 3 + c)] = X[3 * r + c];
        B[ba7_tri(r, 6)] = X[9 + r]; B[ba7_tri(3 + r, 6)] = X[12 + r];
      }
      B[ba7_tri(6, 6)] = Dg[6 * (2 * N + row)];
      ba7_precond_invert(B, s, dd, ff, M, inv);
    }
    for (int i = 0; i < 49; ++i) Mi[i] = inv[i];
  }
}

// ---- PCG on the cameras' 7-vectors (the three nodes of a camera) ----------------------------------------------------------------------
__device__ __forceinline__ void ba7_apply_minv(const double* Mi, const double* r, double* z) {
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    double s = Mi[7 * c] * r[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) s += Mi[7 * c + k] * r[k];
    z[c] = s;
  }
}
// PCG start: y = 0, r = rhs, z = M^-1 r, p = z, q = S p (0 on inactive nodes); zeros in the padding of the intrinsics node
__global__ void k_ba7_pcg_init(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ rhs, const double* __restrict__ Minv,
                               const double* __restrict__ S, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                               double* __restrict__ q) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t N = n_cams;
  double rr[7], zz[7];
  for (int c = 0; c < 7; ++c) rr[c] = rhs[ba7_at(N, k, c)];
  ba7_apply_minv(Minv + 49 * (size_t)k, rr, zz);
  for (int c = 0; c < 7; ++c) {
    const size_t i = ba7_at(N, k, c);
    y[i] = 0.0; r[i] = rr[c]; z[i] = zz[c]; p[i] = zz[c];
    q[i] = active[i / 3] ? S[i] * zz[c] : 0.0;
  }
  const size_t f3 = 3 * (2 * N + k);
  for (int c = 1; c < 3; ++c) { y[f3 + c] = 0.0; r[f3 + c] = 0.0; z[f3 + c] = 0.0; p[f3 + c] = 0.0; q[f3 + c] = 0.0; }
}
// y += alpha p, r -= alpha A p, z = M^-1 r with alpha = rz / pAp from the device scalars (k_ba6_pcg_update with 7 x 7 blocks)
__global__ void k_ba7_pcg_update(uint32_t n_cams, const double* __restrict__ scal, int s_rz, int s_pap, const double* __restrict__ p,
                                 const double* __restrict__ Ap, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z,
                                 const double* __restrict__ Minv) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double pap = scal[s_pap];
  const double alpha = pap > 0.0 ? scal[s_rz] / pap : 0.0;
  const size_t N = n_cams;
  double rr[7], zz[7];
  for (int c = 0; c < 7; ++c) {
    const size_t i = ba7_at(N, k, c);
    y[i] += alpha * p[i]; rr[c] = r[i] - alpha * Ap[i]; r[i] = rr[c];
  }
  ba7_apply_minv(Minv + 49 * (size_t)k, rr, zz);
  for (int c = 0; c < 7; ++c) z[ba7_at(N, k, c)] = zz[c];
  const size_t f3 = 3 * (2 * N + k);
  for (int c = 1; c < 3; ++c) { y[f3 + c] = 0.0; r[f3 + c] = 0.0; z[f3 + c] = 0.0; }
}

// ---- the gauge: the seven directions of gsfm_ba6.h on the orientations, centres and points, nothing on an intrinsics node ---------------
// ba6_gauge_dirs' values without its addressable 7 x 3 array (which costs k_ba6_gauge_dots / k_ba6_gauge_apply 32 bytes of scratch per
// lane): an orientation node has the three rotation directions alone, minus the rows of J_l(w)^-1; a centre or a point has e_c, x - mean
// and e_c x x, whose products are written out.  acc: the 28 entries of the upper triangle of V^T V (row-major), then V^T delta (7).
__device__ __forceinline__ void ba7_gauge_acc_orientation(const double* w, double d0, double d1, double d2, double* acc) {
  double T[9], Ti[9];
  jl_and_inverse(w, T, Ti);
  // v_{4+c} = -(row c of Ti); the signs cancel in the products
  acc[22] += Ti[0] * Ti[0] + Ti[1] * Ti[1] + Ti[2] * Ti[2];   // (4, 4)
  acc[23] += Ti[0] * Ti[3] + Ti[1] * Ti[4] + Ti[2] * Ti[5];   // (4, 5)
  acc[24] += Ti[0] * Ti[6] + Ti[1] * Ti[7] + Ti[2] * Ti[8];   // (4, 6)
  acc[25] += Ti[3] * Ti[3] + Ti[4] * Ti[4] + Ti[5] * Ti[5];   // (5, 5)
  acc[26] += Ti[3] * Ti[6] + Ti[4] * Ti[7] + Ti[5] * Ti[8];   // (5, 6)
  acc[27] += Ti[6] * Ti[6] + Ti[7] * Ti[7] + Ti[8] * Ti[8];   // (6, 6)
  acc[32] -= Ti[0] * d0 + Ti[1] * d1 + Ti[2] * d2;
  acc[33] -= Ti[3] * d0 + Ti[4] * d1 + Ti[5] * d2;
  acc[34] -= Ti[6] * d0 + Ti[7] * d1 + Ti[8] * d2;
}
__device__ __forceinline__ void ba7_gauge_acc_position(double x0, double x1, double x2, double s0, double s1, double s2, double d0, double d1, double d2,
                                                       double* acc) {
  // v0 v1 v2 = e_x e_y e_z, v3 = s = x - mean, v4 = e_x x x = (0, -x2, x1), v5 = e_y x x = (x2, 0, -x0), v6 = e_z x x = (-x1, x0, 0)
  acc[0] += 1.0; acc[3] += s0; acc[5] += x2; acc[6] -= x1;                 // row 0: (0,0) (0,3) (0,5) (0,6)
  acc[7] += 1.0; acc[9] += s1; acc[10] -= x2; acc[12] += x0;               // row 1: (1,1) (1,3) (1,4) (1,6)
  acc[13] += 1.0; acc[14] += s2; acc[15] += x1; acc[16] -= x0;             // row 2: (2,2) (2,3) (2,4) (2,5)
  acc[18] += s0 * s0 + s1 * s1 + s2 * s2;                                  // (3,3)
  acc[19] += -s1 * x2 + s2 * x1; acc[20] += s0 * x2 - s2 * x0; acc[21] += -s0 * x1 + s1 * x0;   // (3,4) (3,5) (3,6)
  acc[22] += x2 * x2 + x1 * x1; acc[23] -= x1 * x0; acc[24] -= x2 * x0;    // (4,4) (4,5) (4,6)
  acc[25] += x2 * x2 + x0 * x0; acc[26] -= x2 * x1;                        // (5,5) (5,6)
  acc[27] += x1 * x1 + x0 * x0;                                            // (6,6)
  acc[28] += d0; acc[29] += d1; acc[30] += d2;
  acc[31] += s0 * d0 + s1 * d1 + s2 * d2;
  acc[32] += -x2 * d1 + x1 * d2; acc[33] += x2 * d0 - x0 * d2; acc[34] += -x1 * d0 + x0 * d1;
}
// part[i * GSFM_POS_PARTS + block]: the block's share of the 35 dots over the active nodes: the orientations first, then the centres and points
__global__ void __launch_bounds__(256) k_ba7_gauge_dots(uint32_t n_cams, size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ x,
                                                         const double* __restrict__ delta, const double* __restrict__ scal, int s_x, double inv_count,
                                                         double* __restrict__ part) {
  __shared__ double lds[5];
  const double m0 = scal[s_x] * inv_count, m1 = scal[s_x + 1] * inv_count, m2 = scal[s_x + 2] * inv_count;
  double acc[GSFM_BA6_GDOTS];
#pragma unroll
  for (int i = 0; i < GSFM_BA6_GDOTS; ++i) acc[i] = 0.0;
  const size_t stride = (size_t)GSFM_POS_PARTS * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x, N = n_cams;
  for (size_t k = first; k < N; k += stride)
    if (active[k]) ba7_gauge_acc_orientation(x + 3 * k, delta[3 * k], delta[3 * k + 1], delta[3 * k + 2], acc);
  for (size_t k = N + first; k < n_nodes; k += stride) {
    if (!active[k] || (k >= 2 * N && k < 3 * N)) continue;   // (an intrinsics node: no direction has a focal component)
    const double x0 = x[3 * k], x1 = x[3 * k + 1], x2 = x[3 * k + 2];
    ba7_gauge_acc_position(x0, x1, x2, x0 - m0, x1 - m1, x2 - m2, delta[3 * k], delta[3 * k + 1], delta[3 * k + 2], acc);
  }
#pragma unroll
  for (int i = 0; i < GSFM_BA6_GDOTS; ++i) {
    const double t = block_sum_bcast(acc[i], lds);
    if (threadIdx.x == 0) part[(size_t)i * GSFM_POS_PARTS + blockIdx.x] = t;
  }
}
// delta -= V c on the active nodes but the intrinsics nodes (c = scal[s_c .. s_c + 6]), cand = x + delta on every node
__global__ void k_ba7_gauge_apply(uint32_t n_cams, size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ x,
                                  const double* __restrict__ scal, int s_x, double inv_count, int s_c, int project, double* __restrict__ delta,
                                  double* __restrict__ cand) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_nodes) return;
  const double x0 = x[3 * k], x1 = x[3 * k + 1], x2 = x[3 * k + 2];
  double d0 = delta[3 * k], d1 = delta[3 * k + 1], d2 = delta[3 * k + 2];
  const bool intrinsics_node = k >= 2 * (size_t)n_cams && k < 3 * (size_t)n_cams;
  if (project && active[k] && !intrinsics_node) {
    const double c4 = scal[s_c + 4], c5 = scal[s_c + 5], c6 = scal[s_c + 6];
    if (k < n_cams) {   // v_{4+c} = -(row c of J_l(w)^-1)
      double T[9], Ti[9];
      jl_and_inverse(x + 3 * k, T, Ti);
      d0 += c4 * Ti[0] + c5 * Ti[3] + c6 * Ti[6];
      d1 += c4 * Ti[1] + c5 * Ti[4] + c6 * Ti[7];
      d2 += c4 * Ti[2] + c5 * Ti[5] + c6 * Ti[8];
    } else {
      const double c3 = scal[s_c + 3];
      const double s0 = x0 - scal[s_x] * inv_count, s1 = x1 - scal[s_x + 1] * inv_count, s2 = x2 - scal[s_x + 2] * inv_count;
      d0 -= scal[s_c] + c3 * s0 + c5 * x2 - c6 * x1;
      d1 -= scal[s_c + 1] + c3 * s1 - c4 * x2 + c6 * x0;
      d2 -= scal[s_c + 2] + c3 * s2 + c4 * x1 - c5 * x0;
    }
  }
  delta[3 * k] = d0; delta[3 * k + 1] = d1; delta[3 * k + 2] = d2;
  cand[3 * k] = x0 + d0; cand[3 * k + 1] = x1 + d1; cand[3 * k + 2] = x2 + d2;
}

}  // namespace gsfm
