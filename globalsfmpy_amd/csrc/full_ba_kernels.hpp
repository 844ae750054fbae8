// Device kernels of the full bundle adjustment, one family for both of its forms, parameterised by the camera dimension D:
//   D = 6 (include/gsfm_ba6.h): camera orientations, camera positions and points move together;
//   D = 7 (include/gsfm_ba7.h): the focal lengths move too, a seventh coordinate per camera.
//
// Structure.  With free orientations an observation's camera Jacobian is Jc = [Jr, -Jp] (2 x 6: the corrected Jacobians with respect to the
// angle-axis vector and, with J_pos = -J_point, to the centre) or Jc = [Jr, -Jp, Jf] (2 x 7), so the normal matrix has D x D camera blocks and
// D x 3 off-diagonal blocks and ba_kernels.hpp's block Laplacian is gone.  The products run MATRIX-FREE on the corrected Jacobians: per
// observation Jp (6 doubles), Jr (6) and, at D = 7, Jf (2): D 16-byte pieces, 96 or 112 bytes per pass -- the stream of ba_kernels.hpp's H_e
// twice over, where the formed blocks Jc^T Jc, Jc^T Jp, Jp^T Jp would be 45 doubles:  (J d)_e = Jr d_rot + Jp (d_point - d_pos) [+ Jf d_f].
//
// Unknowns are one array of (NODES n_cams + n_tracks) x 3 with NODES = 2 or 3 nodes per camera: the cameras' angle-axis vectors, the cameras'
// centres, at D = 7 the cameras' INTRINSICS NODES (f, 0, 0), the points -- three or four kinds of 3-vector nodes, so that the node-wise
// kernels of pos_kernels.hpp and ba_kernels.hpp (dots, norms, reductions, Jacobi scale, D^2, the PCG direction, k_ba_scale) run unchanged;
// the points' inverses are this file's (k_ba6_prep_points: kept and applied in double-double).  (The two spare coordinates of an intrinsics
// node leave room for k1 k2.)  `active` has one byte per node: a camera's first two nodes carry the camera's byte, its intrinsics node carries
// `camera active && focal_free`; a held focal length is thereby no parameter: it enters no norm, gets a zero step from k_ba_scale and a zero q
// from k_pos_pcg_dir, and the kernels below read its value from x like any other.
// INVARIANT: the two padding coordinates of an intrinsics node are exact zeros (+0 or -0) in every vector that a dot, a norm or the gauge
// sums read: x, cand, g, b, y, delta, rhs, r, z, p, q, Ap.  x gets them from the upload; every kernel here that writes one of the others
// writes the zeros itself (k_fba_cam_lin: g and Dg; k_fba_cam_pass: rhs and Ap; k_fba_pcg_init / k_fba_pcg_update: y, r, z, p, q); the
// node-wise kernels keep them (S = 1 and D^2 = min_lm_diagonal / radius there multiply zeros only).  The same holds for the focal
// coordinate of a camera whose focal length is held.
// Dg holds the 3 x 3 diagonal blocks per node, (B_ff, 0, 0, 0, 0, 0) on an intrinsics node; the blocks between a camera's nodes go to Bx
// (for gsfm_ba*_linearize, and for the last resort of k_fba_cam_precond), Fba<D>::BX doubles per camera: w x o (9, row-major) and, at D = 7,
// w x f (3), o x f (3), one spare.
//
// Layout.  Per observation in the caller's (track-major) order: Jt (Fba<D>::J doubles: Jp rows 0 1, Jr rows 0 1, at D = 7 Jf) and Rt (2: r~),
// written by the POINT side of the linearisation, the only place that evaluates an observation.  The camera side copies Jt into its own
// order, Jc (one gather per observation per linearisation), and reads Rt.  The camera records (k_fba_cameras: R(w), f u v, the estimated
// flag and J_l(w), O(n_cams)) are rebuilt at every evaluation point, so that no observation pays for a sincos; at D = 7 the record's f is the
// evaluation point's, not that of `intrinsics`.
//
// Lane groups, row-per-wavefront, loop bounds, shuffles and the absence of atomics and of waits are those of ba_kernels.hpp.
// The gauge kernels exist per form (k_ba6_gauge_*, k_ba7_gauge_*): the two associate their sums differently.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ba_kernels.hpp"
#include "so3_dev.hpp"

namespace gsfm {

#define GSFM_BA6_CAM_DOUBLES 32   // R (9), unused (3), f u v, estimated (the record of k_tri_cameras), then J_l(w) (9) and padding to 256 bytes
#define GSFM_BA6_GAUGE 7          // translations (3), scale, rotations (3)
#define GSFM_BA6_GDOTS 35         // the upper triangle of V^T V (28, row-major) and V^T delta (7)
#define GSFM_BA7_BX 16

// what follows from the camera dimension
template <int D> struct Fba {
  static_assert(D == 6 || D == 7, "the camera dimension is 6 (w, o) or 7 (w, o, f)");
  static constexpr int NODES = D == 6 ? 2 : 3;       // nodes per camera
  static constexpr int J = 2 * D;                    // doubles per observation: Jp rows 0 1 (6), Jr rows 0 1 (6)[, Jf (2)]
  static constexpr int TRI = D * (D + 1) / 2;        // the upper triangle of a D x D, row-major
  static constexpr int BX = D == 6 ? 9 : GSFM_BA7_BX;
};

struct FbaDev {
  BaDev b;           // n_cams, n_tracks, the CSRs, track_used, active (NODES N + T bytes), leaf; cams: GSFM_BA6_CAM_DOUBLES per camera; Ht, At, Hc unused
  double* Jt;        // n_obs x J in track order (zero for an unused observation)
  double* Rt;        // n_obs x 2: r~
  double* Jc;        // n_used x J: Jt in camera order
};

template <int D> __device__ __forceinline__ void fba_load_j(const double* J, size_t i, double* j) {
  const double2* jp = (const double2*)(J + Fba<D>::J * i);
#pragma unroll
  for (int k = 0; k < D; ++k) { const double2 v = jp[k]; j[2 * k] = v.x; j[2 * k + 1] = v.y; }
}
template <int D> __device__ __forceinline__ void fba_store_j(double* J, size_t i, const double* j) {
  double2* jp = (double2*)(J + Fba<D>::J * i);
#pragma unroll
  for (int k = 0; k < D; ++k) jp[k] = make_double2(j[2 * k], j[2 * k + 1]);
}
// the rows of Jc = [Jr, -Jp(, Jf)] for j = (Jp0, Jp1, Jr0, Jr1(, Jf))
template <int D> __device__ __forceinline__ void fba_rows(const double* j, double* c0, double* c1) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { c0[c] = j[6 + c]; c1[c] = j[9 + c]; c0[3 + c] = -j[c]; c1[3 + c] = -j[3 + c]; }
  if constexpr (D == 7) { c0[6] = j[12]; c1[6] = j[13]; }
}
// u = Jr a + Jp b (+ Jf f) (2-vector)
template <int D> __device__ __forceinline__ void fba_apply(const double* j, const double* a, const double* b, double f, double& u0, double& u1) {
  u0 = j[6] * a[0] + j[7] * a[1] + j[8] * a[2] + j[0] * b[0] + j[1] * b[1] + j[2] * b[2];
  u1 = j[9] * a[0] + j[10] * a[1] + j[11] * a[2] + j[3] * b[0] + j[4] * b[1] + j[5] * b[2];
  if constexpr (D == 7) { u0 += j[12] * f; u1 += j[13] * f; }
}
// the index of coordinate c (w, o(, f)) of camera `row` in a node vector
template <int D> __host__ __device__ __forceinline__ size_t fba_at(size_t n_cams, size_t row, int c) {
  return c < 3 ? 3 * row + c : (D == 6 || c < 6) ? 3 * (n_cams + row) + (c - 3) : 3 * (2 * n_cams + row);
}
template <int D> __device__ __forceinline__ constexpr int fba_tri(int r, int c) { return r * D - r * (r - 1) / 2 + (c - r); }   // r <= c

// The camera records at the evaluation point `at` (its first n_cams nodes are the angle-axis vectors; D = 7: f from the camera's intrinsics node).
template <int D>
__global__ void __launch_bounds__(256) k_fba_cameras(uint32_t n_cams, const double* __restrict__ at, const double* __restrict__ intrinsics,
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
  o[12] = D == 7 ? at[3 * (2 * (size_t)n_cams + c)] : intrinsics[3 * (size_t)c];
  o[13] = intrinsics[3 * (size_t)c + 1]; o[14] = intrinsics[3 * (size_t)c + 2];
  o[15] = cam_estimated[c] ? 1.0 : 0.0;
#pragma unroll
  for (int k = 25; k < GSFM_BA6_CAM_DOUBLES; ++k) o[k] = 0.0;
}

// (the double-double pieces of the point solve -- ba6_two_sum .. ba6_apply_inv_dd, ba6_refine_inv3 -- are in ba_kernels.hpp, which uses them too)

// ---- point side ------------------------------------------------------------------------------------------------------------------
// Linearisation at x: per observation Jp, Jr(, Jf) and r~ (stored in track order), per point C_t = sum Jp^T Jp into Dg and g_t = sum Jp^T r~ into g.
template <int D, int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_fba_lin_tracks(FbaDev af, BaSlots sl, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const BaDev& a = af.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = Fba<D>::NODES * N + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_BA6_CAM_DOUBLES * c;
    double j[Fba<D>::J] = {}, r0 = 0.0, r1 = 0.0;
    if (used_t && cam[15] != 0.0) {
      double rho0;
      const double* o = x + 3 * (N + c);
      reproj_corrected_free<D == 7>(cam, cam + 16, a.obs_xy[e], X[0] - o[0], X[1] - o[1], X[2] - o[2], a.leaf, j, j + 3, j + 6, j + 9, j + 12, r0, r1, rho0);
      s[0] += j[0] * j[0] + j[3] * j[3]; s[1] += j[0] * j[1] + j[3] * j[4]; s[2] += j[0] * j[2] + j[3] * j[5];
      s[3] += j[1] * j[1] + j[4] * j[4]; s[4] += j[1] * j[2] + j[4] * j[5]; s[5] += j[2] * j[2] + j[5] * j[5];
      s[6] += j[0] * r0 + j[3] * r1; s[7] += j[1] * r0 + j[4] * r1; s[8] += j[2] * r0 + j[5] * r1;
    }
    fba_store_j<D>(af.Jt, e, j);
    *(double2*)(af.Rt + 2 * e) = make_double2(r0, r1);
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

// Cost at x (the records hold R, and at D = 7 f, of x): cost_t[t] = sum over the track's used observations of rho(|r|^2) / 2.  The points are
// the nodes from n_cam_nodes on.  r_out (n_obs x 2) and rho_out (n_obs), for gsfm_ba*_residuals, may be NULL; an unused observation gets zeros.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_fba_cost_tracks(FbaDev af, BaSlots sl, size_t n_cam_nodes, const double* __restrict__ x, double* __restrict__ cost_t,
                                                           double* __restrict__ r_out, double* __restrict__ rho_out) {
  const BaDev& a = af.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = n_cam_nodes + tk.t;
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
// on the cameras' nodes (0 on inactive ones, a held focal length's included), add = the node vector b or NULL.  scaled_out: out_t = S_t u_t
// (the z_t the camera pass gathers), else u_t.
//   Schur product      sgn = +1, add = NULL, scaled:  z = S C~^-1 E~^T v
//   back-substitution  sgn = -1, add = b:             y_p = C~^-1 (b_p - E~^T y_c)
template <int D, int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_fba_point_pass(FbaDev af, BaSlots sl, const double* __restrict__ q, const double* __restrict__ S,
                                                          const double* __restrict__ Cinv, const double* __restrict__ add, double sgn,
                                                          double* __restrict__ out, int scaled_out) {
  const BaDev& a = af.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams;
  double yh[3] = {0.0, 0.0, 0.0}, yl[3] = {0.0, 0.0, 0.0};   // the track sums in double-double
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[Fba<D>::J];
    fba_load_j<D>(af.Jt, e, j);
    const double* qr = q + 3 * c, * qp = q + 3 * (N + c);
    // u = Jc q = Jr q_rot - Jp q_pos (+ Jf q_f)
    double uh[2] = {0.0, 0.0}, ul[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { ba6_dd_mac(j[6 + 3 * r + i], qr[i], uh[r], ul[r]); ba6_dd_mac(-j[3 * r + i], qp[i], uh[r], ul[r]); }
      if constexpr (D == 7) ba6_dd_mac(j[12 + r], q[3 * (2 * N + c)], uh[r], ul[r]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { ba6_dd_mac2(j[i], uh[0], ul[0], yh[i], yl[i]); ba6_dd_mac2(j[3 + i], uh[1], ul[1], yh[i], yl[i]); }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) ba6_group_allsum_dd<G>(yh[i], yl[i]);
  if (tk.live && l == 0) {
    const size_t node = Fba<D>::NODES * N + tk.t;
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

// quad_t[t] = sum_{e in t} |J~_e delta|^2 with J~_e delta = Jr d_rot + Jp (d_t - d_pos) (+ Jf d_f); jd_out (n_obs x 2, may be NULL) gets J~_e delta
template <int D, int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_fba_quad_tracks(FbaDev af, BaSlots sl, const double* __restrict__ delta, double* __restrict__ quad_t,
                                                           double* __restrict__ jd_out) {
  const BaDev& a = af.b;
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t N = a.n_cams, node = Fba<D>::NODES * N + tk.t;
  double d[3] = {0.0, 0.0, 0.0};
  if (tk.live) { d[0] = delta[3 * node]; d[1] = delta[3 * node + 1]; d[2] = delta[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double j[Fba<D>::J];
    fba_load_j<D>(af.Jt, e, j);
    const double* dp = delta + 3 * (N + c);
    const double v[3] = {d[0] - dp[0], d[1] - dp[1], d[2] - dp[2]};
    double df = 0.0, u0, u1;
    if constexpr (D == 7) df = delta[3 * (2 * N + c)];
    fba_apply<D>(j, delta + 3 * c, v, df, u0, u1);
    acc += u0 * u0 + u1 * u1;
    if (jd_out) { jd_out[2 * e] = u0; jd_out[2 * e + 1] = u1; }
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) quad_t[tk.t] = acc;
}

// ---- camera side: one wavefront per row -------------------------------------------------------------------------------------------
// The camera half of the linearisation: the row's Jacobians copied into camera order, g_k = sum Jc^T r~ (D) and B_k = sum Jc^T Jc (the TRI
// entries of its upper triangle), scattered to g, Dg and Bx.  A held focal length gets zeros in its entry, row and column.
template <int D>
__global__ void __launch_bounds__(256) k_fba_cam_lin(FbaDev af, double* __restrict__ g, double* __restrict__ Dg, double* __restrict__ Bx) {
  constexpr int TRI = Fba<D>::TRI;
  const BaDev& a = af.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  double acc[D + TRI];
#pragma unroll
  for (int q = 0; q < D + TRI; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t e = a.cobs[d];
    double j[Fba<D>::J];
    fba_load_j<D>(af.Jt, e, j);
    fba_store_j<D>(af.Jc, d, j);
    const double2 r = *(const double2*)(af.Rt + 2 * e);
    if constexpr (D == 6) {
      // gsfm_ba6's results are pinned bit for bit to sums that subtract the products with Jp; the compiler contracts acc -= a b + c d and
      // acc += (-a) b + (-c) d differently (which product is rounded before the fused one), so this form stays beside the one on Jc's rows
      const double* p0 = j, * p1 = j + 3, * q0 = j + 6, * q1 = j + 9;
      double* B = acc + D;
#pragma unroll
      for (int c = 0; c < 3; ++c) { acc[c] += q0[c] * r.x + q1[c] * r.y; acc[3 + c] -= p0[c] * r.x + p1[c] * r.y; }
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
        for (int c = rr; c < 3; ++c) {
          B[fba_tri<D>(rr, c)] += q0[rr] * q0[c] + q1[rr] * q1[c];
          B[fba_tri<D>(3 + rr, 3 + c)] += p0[rr] * p0[c] + p1[rr] * p1[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) B[fba_tri<D>(rr, 3 + c)] -= q0[rr] * p0[c] + q1[rr] * p1[c];
      }
    } else {
      double c0[D], c1[D];
      fba_rows<D>(j, c0, c1);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] += c0[c] * r.x + c1[c] * r.y;
      int q = D;
#pragma unroll
      for (int rr = 0; rr < D; ++rr)
#pragma unroll
        for (int c = rr; c < D; ++c) acc[q++] += c0[rr] * c0[c] + c1[rr] * c1[c];
    }
  }
#pragma unroll
  for (int q = 0; q < D + TRI; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    const size_t N = a.n_cams, kr = row, kp = N + row;
    const double* B = acc + D;
    double* X = Bx + Fba<D>::BX * (size_t)row;
    for (int c = 0; c < 3; ++c) { g[3 * kr + c] = acc[c]; g[3 * kp + c] = acc[3 + c]; }
    int q = 0;
    for (int r = 0; r < 3; ++r)
      for (int c = r; c < 3; ++c) { Dg[6 * kr + q] = B[fba_tri<D>(r, c)]; Dg[6 * kp + q] = B[fba_tri<D>(3 + r, 3 + c)]; ++q; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) X[3 * r + c] = B[fba_tri<D>(r, 3 + c)];
    if constexpr (D == 7) {
      const size_t kf = 2 * N + row;
      const double ff = a.active[kf] ? 1.0 : 0.0;   // (a held focal length: exact zeros)
      g[3 * kf] = ff * acc[6]; g[3 * kf + 1] = 0.0; g[3 * kf + 2] = 0.0;
      Dg[6 * kf] = ff * B[fba_tri<D>(6, 6)];
      for (int c = 1; c < 6; ++c) Dg[6 * kf + c] = 0.0;
      for (int r = 0; r < 3; ++r) { X[9 + r] = ff * B[fba_tri<D>(r, 6)]; X[12 + r] = ff * B[fba_tri<D>(3 + r, 6)]; }
      X[15] = 0.0;
    }
  }
}

// The camera pass:  out_k = S_k sum_{e in k} Jc^T (Jc q_k - Jp zs z_{t(e)}) + D2_k p_k + add_k  on active rows (q, p, add may be NULL: zero),
// written to the row's nodes.  On an inactive row and on a held focal coordinate: p_k when identity_inactive (the PCG operator is the identity
// there), else 0.  The padding of the intrinsics node gets zeros.
//   Schur product   q = S p, z from the point pass, zs = 1:  out = Sc p
//   reduced rhs     q = NULL, z = -S C~^-1 b_p (k_ba6_prep_points), zs = -1, add = b:  out = b_c - E~ C~^-1 b_p
template <int D>
__global__ void __launch_bounds__(256) k_fba_cam_pass(FbaDev af, const double* __restrict__ q, const double* __restrict__ z, double zs,
                                                       const double* __restrict__ p, const double* __restrict__ S, const double* __restrict__ D2,
                                                       const double* __restrict__ add, double* __restrict__ out, int identity_inactive) {
  const BaDev& a = af.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t N = a.n_cams, f3 = 3 * (2 * N + row);   // (f3: the intrinsics node, D = 7)
  if (!a.active[row]) {
    if (lane < D) { const size_t i = fba_at<D>(N, row, lane); out[i] = (identity_inactive && p) ? p[i] : 0.0; }
    if constexpr (D == 7) if (lane == 0) { out[f3 + 1] = 0.0; out[f3 + 2] = 0.0; }
    return;
  }
  double qq[D] = {};
  if (q) {
#pragma unroll
    for (int c = 0; c < D; ++c) qq[c] = q[fba_at<D>(N, row, c)];
  }
  double y[D] = {};
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t t = a.ctrk[d];
    double j[Fba<D>::J];
    fba_load_j<D>(af.Jc, d, j);
    const double v[3] = {-(qq[3] + zs * z[3 * t]), -(qq[4] + zs * z[3 * t + 1]), -(qq[5] + zs * z[3 * t + 2])};
    double u0, u1;
    fba_apply<D>(j, qq, v, qq[D - 1], u0, u1);
    if constexpr (D == 6) {   // (the form gsfm_ba6's bytes are pinned to: k_fba_cam_lin)
#pragma unroll
      for (int c = 0; c < 3; ++c) { y[c] += j[6 + c] * u0 + j[9 + c] * u1; y[3 + c] -= j[c] * u0 + j[3 + c] * u1; }
    } else {
      double c0[D], c1[D];
      fba_rows<D>(j, c0, c1);
#pragma unroll
      for (int c = 0; c < D; ++c) y[c] += c0[c] * u0 + c1[c] * u1;
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) y[c] = wave_sum(y[c]);
  if (lane == 0) {
    bool ff = true;
    if constexpr (D == 7) ff = a.active[2 * N + row] != 0;
    for (int c = 0; c < D; ++c) {
      const size_t i = fba_at<D>(N, row, c);
      double o = S[i] * y[c];
      if (p) o += D2[i] * p[i];
      if (add) o += add[i];
      if (c == 6 && !ff) o = (identity_inactive && p) ? p[i] : 0.0;
      out[i] = o;
    }
    if constexpr (D == 7) { out[f3 + 1] = 0.0; out[f3 + 2] = 0.0; }
  }
}

// Cholesky M = L L^T of a symmetric positive definite D x D (full, row-major) and Minv = L^-T L^-1, in one lane.  false: a pivot was not
// positive (or not finite) -- M is not positive definite as computed and Minv is not to be used.
template <int D> __device__ __forceinline__ bool fba_inv_spd(const double* M, double* Minv) {
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
  // Li = L^-1 (lower triangular), column by column
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

// The preconditioner, the D x D block diagonal of the Schur complement (Ceres' SCHUR_JACOBI), inverted per camera:
//   M_k = S_k (sum_{e in k} Jc^T (I - Jp G_t Jp^T) Jc) S_k + D2_k,   G_t = S_t C~_t^-1 S_t;   the identity on inactive rows.
// G_t is plain fp64.  Where a point's block has lost rank (beyond the Tukey cut: one observation left) and is held up by the damping alone
// (1e-10 of its scaled diagonal at radius 1e10), Jp G_t Jp^T carries u cond(C~_t), W = I - Jp G_t Jp^T (of the damping's size) is noise and M_k
// can come out indefinite: its Cholesky fails.  Such a row is summed again with W from the pair inverse of k_ba6_prep_points, 1 - t^T C~^-1 t
// accumulated in double-double (t = S_t Jp^T); should that block fail too, the row takes the block of B~ alone, S_k B_k S_k + D2_k (Dg and Bx of
// k_fba_cam_lin), positive definite by the damping.  Rows whose first Cholesky succeeds keep their bytes.  (Before, the NaNs of the failed
// factorisation made r.z NaN and the PCG returned y = 0 without a word.)
// A held focal coordinate is decoupled (zero row and column, diagonal 1): the other six get the numbers of D = 6.
template <int D> __device__ __forceinline__ void fba_precond_add(const double* j, double w00, double w01, double w11, double* acc) {
  // the rows of Jc and of W Jc
  double c0[D], c1[D], d0[D], d1[D];
  fba_rows<D>(j, c0, c1);
#pragma unroll
  for (int c = 0; c < D; ++c) { d0[c] = w00 * c0[c] + w01 * c1[c]; d1[c] = w01 * c0[c] + w11 * c1[c]; }
  int q = 0;
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = r; c < D; ++c) acc[q++] += c0[r] * d0[c] + c1[r] * d1[c];
}
// M = S acc S + D2 from the TRI sums (D = 7 and focal_free = false: the focal coordinate decoupled), inverted
template <int D> __device__ __forceinline__ bool fba_precond_invert(const double* acc, const double* s, const double* dd, bool focal_free, double* M, double* inv) {
  int q = 0;
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = r; c < D; ++c) {
      double m = s[r] * acc[q++] * s[c] + (r == c ? dd[r] : 0.0);
      if (c == 6 && !focal_free) m = r == 6 ? 1.0 : 0.0;
      M[D * r + c] = m; M[D * c + r] = m;
    }
  return fba_inv_spd<D>(M, inv);
}
template <int D>
__global__ void __launch_bounds__(256) k_fba_cam_precond(FbaDev af, const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ Gt,
                                                          const double* __restrict__ Cinv, const double* __restrict__ Dg, const double* __restrict__ Bx,
                                                          double* __restrict__ Minv) {
  constexpr int TRI = Fba<D>::TRI;
  const BaDev& a = af.b;
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  double* Mi = Minv + D * D * (size_t)row;
  if (!a.active[row]) {
    if (lane < D * D) Mi[lane] = (lane % (D + 1) == 0) ? 1.0 : 0.0;
    return;
  }
  const size_t N = a.n_cams;
  bool ff = true;
  if constexpr (D == 7) ff = a.active[2 * N + row] != 0;
  double acc[TRI];
#pragma unroll
  for (int q = 0; q < TRI; ++q) acc[q] = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[Fba<D>::J], gt[6];
    fba_load_j<D>(af.Jc, d, j);
    ba_load_h(Gt, a.ctrk[d], gt);
    // W = I - Jp G Jp^T (2 x 2, symmetric)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    ba_sym_mac(gt, j[0], j[1], j[2], a0, a1, a2);
    ba_sym_mac(gt, j[3], j[4], j[5], b0, b1, b2);
    const double w00 = 1.0 - (j[0] * a0 + j[1] * a1 + j[2] * a2), w01 = -(j[0] * b0 + j[1] * b1 + j[2] * b2), w11 = 1.0 - (j[3] * b0 + j[4] * b1 + j[5] * b2);
    fba_precond_add<D>(j, w00, w01, w11, acc);
  }
#pragma unroll
  for (int q = 0; q < TRI; ++q) acc[q] = wave_sum(acc[q]);
  double s[D], dd[D];
#pragma unroll
  for (int c = 0; c < D; ++c) { const size_t i = fba_at<D>(N, row, c); s[c] = S[i]; dd[c] = D2[i]; }
  int ok = 1;
  if (lane == 0) {
    double M[D * D], inv[D * D];
    ok = fba_precond_invert<D>(acc, s, dd, ff, M, inv) ? 1 : 0;
    if (ok) for (int i = 0; i < D * D; ++i) Mi[i] = inv[i];
  }
  if (__shfl(ok, 0, 64)) return;   // (wave-uniform)
  // the row again, W through the pair inverse
#pragma unroll
  for (int q = 0; q < TRI; ++q) acc[q] = 0.0;
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double j[Fba<D>::J];
    fba_load_j<D>(af.Jc, d, j);
    const size_t t = a.ctrk[d], node = Fba<D>::NODES * N + t;
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
    fba_precond_add<D>(j, -(h00 + l00), -(h01 + l01), -(h11 + l11), acc);
  }
#pragma unroll
  for (int q = 0; q < TRI; ++q) acc[q] = wave_sum(acc[q]);
  if (lane == 0) {
    double M[D * D], inv[D * D];
    if (!fba_precond_invert<D>(acc, s, dd, ff, M, inv)) {
      // Last resort, reached by no test since the row is summed again above: B~'s block, S_k B_k S_k + D2_k from Dg and Bx (a held focal length
      // has zeros there already), is positive definite by construction (a sum of Jc^T Jc plus D2 > 0), so the result of its factorisation is
      // not looked at; NaN inputs stay NaN and end as a stall in the PCG.
      const double* Dr = Dg + 6 * (size_t)row, * Dp = Dg + 6 * (N + row), * X = Bx + Fba<D>::BX * (size_t)row;
      double B[TRI];
      int q = 0;
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) { B[fba_tri<D>(r, c)] = Dr[q]; B[fba_tri<D>(3 + r, 3 + c)] = Dp[q]; ++q; }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) B[fba_tri<D>(r, 3 + c)] = X[3 * r + c];
      if constexpr (D == 7) {
        for (int r = 0; r < 3; ++r) { B[fba_tri<D>(r, 6)] = X[9 + r]; B[fba_tri<D>(3 + r, 6)] = X[12 + r]; }
        B[fba_tri<D>(6, 6)] = Dg[6 * (2 * N + row)];
      }
      fba_precond_invert<D>(B, s, dd, ff, M, inv);
    }
    for (int i = 0; i < D * D; ++i) Mi[i] = inv[i];
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

// ---- PCG on the cameras' D-vectors (the nodes of a camera) -----------------------------------------------------------------------------
template <int D> __device__ __forceinline__ void fba_apply_minv(const double* Mi, const double* r, double* z) {
#pragma unroll
  for (int c = 0; c < D; ++c) {
    double s = Mi[D * c] * r[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s += Mi[D * c + k] * r[k];
    z[c] = s;
  }
}
// PCG start: y = 0, r = rhs, z = M^-1 r, p = z, q = S p (0 on inactive nodes); zeros in the padding of the intrinsics node
template <int D>
__global__ void k_fba_pcg_init(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ rhs, const double* __restrict__ Minv,
                               const double* __restrict__ S, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                               double* __restrict__ q) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t N = n_cams;
  double rr[D], zz[D];
  for (int c = 0; c < D; ++c) rr[c] = rhs[fba_at<D>(N, k, c)];
  fba_apply_minv<D>(Minv + D * D * (size_t)k, rr, zz);
  for (int c = 0; c < D; ++c) {
    const size_t i = fba_at<D>(N, k, c);
    y[i] = 0.0; r[i] = rr[c]; z[i] = zz[c]; p[i] = zz[c];
    q[i] = active[c < 6 ? k : 2 * N + k] ? S[i] * zz[c] : 0.0;   // (a camera's first two nodes carry the camera's byte)
  }
  if constexpr (D == 7) {
    const size_t f3 = 3 * (2 * N + k);
    for (int c = 1; c < 3; ++c) { y[f3 + c] = 0.0; r[f3 + c] = 0.0; z[f3 + c] = 0.0; p[f3 + c] = 0.0; q[f3 + c] = 0.0; }
  }
}
// y += alpha p, r -= alpha A p, z = M^-1 r with alpha = rz / pAp from the device scalars (k_pos_pcg_update with D x D blocks)
template <int D>
__global__ void k_fba_pcg_update(uint32_t n_cams, const double* __restrict__ scal, int s_rz, int s_pap, const double* __restrict__ p,
                                 const double* __restrict__ Ap, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z,
                                 const double* __restrict__ Minv) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const double pap = scal[s_pap];
  const double alpha = pap > 0.0 ? scal[s_rz] / pap : 0.0;
  const size_t N = n_cams;
  double rr[D], zz[D];
  for (int c = 0; c < D; ++c) {
    const size_t i = fba_at<D>(N, k, c);
    y[i] += alpha * p[i]; rr[c] = r[i] - alpha * Ap[i]; r[i] = rr[c];
  }
  fba_apply_minv<D>(Minv + D * D * (size_t)k, rr, zz);
  for (int c = 0; c < D; ++c) z[fba_at<D>(N, k, c)] = zz[c];
  if constexpr (D == 7) {
    const size_t f3 = 3 * (2 * N + k);
    for (int c = 1; c < 3; ++c) { y[f3 + c] = 0.0; r[f3 + c] = 0.0; z[f3 + c] = 0.0; }
  }
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

// ---- the gauge at D = 7: the same seven directions on the orientations, centres and points, nothing on an intrinsics node ----------------
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
