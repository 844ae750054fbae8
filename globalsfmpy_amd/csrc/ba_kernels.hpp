// Device kernels of the bundle adjustment of camera positions and points with fixed orientations (include/gsfm_ba.h): Theia's
// BundleAdjustCameraPositionsAndPoints under the definition of that header.
//
// Structure.  With p = R_k (X_t - o_k) an observation's camera Jacobian is minus its point Jacobian J~, so with H_e = J~^T J~ (3 x 3,
// symmetric) and a_e = J~^T r~ the normal matrix is a block graph Laplacian on the bipartite camera / point graph: camera blocks B_k =
// sum_{e in k} H_e, point blocks C_t = sum_{e in t} H_e, off-diagonal blocks -H_e; gradient g_k = -sum a_e, g_t = +sum a_e.  The blocks
// are kept UNSCALED; the Jacobi scale S and the damping D^2 are vector operations around the products (as in pos_kernels.hpp), so the
// scaled off-diagonal block is E~_e = -S_k H_e S_t without ever being stored.
//
// Unknowns are one array of (n_cams + n_tracks) x 3: the cameras' positions, then the points.  `active` has one byte per such node.
//
// Layout.  Per observation, in the caller's (track-major) order: Ht (6 doubles, 00 01 02 11 12 22) and At (3), written by the POINT side
// of the linearisation, the only place that evaluates an observation's Jacobian.  The camera side copies Ht into its own order, Hc (one
// 48-byte gather per observation per LINEARISATION), and reads At.  Both passes of the Schur product then stream their blocks; they
// gather only the 24-byte vectors q_k (point pass) and z_t (camera pass).
//
//   point side   a track is worked by a lane group of G = 4 / 16 / 64 lanes by its CSR length, in gsfm_tracks_launch_order's order, lane l
//                taking the observations l, l + G, ... and an xor butterfly giving every lane the sums (triangulate_kernels.hpp).
//   camera side  one wavefront per camera row, lanes stride the row, a fixed shuffle tree (wave_sum) per row.
// Every loop is bounded by a CSR length known at launch, no kernel waits for another work-group, every shuffle is executed by all lanes
// of its wavefront (idle groups run along on an empty track), and there are no atomics: every sum has a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pos_kernels.hpp"
#include "triangulate_kernels.hpp"
#include "reproj_dev.hpp"

namespace gsfm {

struct BaDev {
  uint32_t n_cams;
  uint32_t n_tracks;
  const uint64_t* track_ptr;   // T + 1
  const uint32_t* obs_cam;     // per observation
  const double2* obs_xy;       // pixels
  const double* cams;          // GSFM_TRI_CAM_DOUBLES per camera (k_tri_cameras; the position field is not read: positions are unknowns)
  const uint8_t* track_used;   // T: the track is estimated
  const uint32_t* crow_ptr;    // N + 1: the camera CSR of the used observations (ba_structure.hpp)
  const uint32_t* cobs;        // its observation ...
  const uint32_t* ctrk;        // ... and track per entry
  const uint8_t* active;       // N + T
  double* Ht;                  // n_obs x 6: H_e in track order (zero for an unused observation)
  double* At;                  // n_obs x 3: a_e
  double* Hc;                  // n_used x 6: H_e in camera order
  DevLossNode leaf;            // the one simple leaf of the loss (TRIVIAL for the NULL loss)
};

// one lane class's slice of the launch order
struct BaSlots {
  uint64_t n_slots;
  const uint32_t* order;
};

struct BaTrack {
  bool live;
  uint32_t t;
  uint64_t ob;
  uint32_t len;
};
template <int G>
__device__ __forceinline__ BaTrack ba_track(const BaDev& a, const BaSlots& s) {
  constexpr int GROUPS = (G == 64 ? 64 : GSFM_TRI_BLOCK) / G;
  BaTrack k;
  const uint64_t slot = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / G;
  k.live = slot < s.n_slots;
  k.t = k.live ? s.order[slot] : 0u;
  k.ob = k.live ? a.track_ptr[k.t] : 0;
  k.len = k.live ? (uint32_t)(a.track_ptr[k.t + 1] - k.ob) : 0u;   // a dead group runs along on an empty track
  return k;
}
#define GSFM_BA_TRACK_BOUNDS(G) __launch_bounds__(G == 64 ? 64 : GSFM_TRI_BLOCK)

__device__ __forceinline__ void ba_load_h(const double* H, size_t i, double* h) {
  const double2* hp = (const double2*)(H + 6 * i);
  const double2 h01 = hp[0], h23 = hp[1], h45 = hp[2];
  h[0] = h01.x; h[1] = h01.y; h[2] = h23.x; h[3] = h23.y; h[4] = h45.x; h[5] = h45.y;
}
__device__ __forceinline__ void ba_store_h(double* H, size_t i, const double* h) {
  double2* hp = (double2*)(H + 6 * i);
  hp[0] = make_double2(h[0], h[1]); hp[1] = make_double2(h[2], h[3]); hp[2] = make_double2(h[4], h[5]);
}
// y += H v, H symmetric (00 01 02 11 12 22)
__device__ __forceinline__ void ba_sym_mac(const double* h, double v0, double v1, double v2, double& y0, double& y1, double& y2) {
  y0 += h[0] * v0 + h[1] * v1 + h[2] * v2;
  y1 += h[1] * v0 + h[3] * v1 + h[4] * v2;
  y2 += h[2] * v0 + h[4] * v1 + h[5] * v2;
}

// ---- double-double pieces (the point solve) ------------------------------------------------------------------------------------------
// Far from the minimum a point's damped block C~_t can be nearly singular.  Its inverse then has entries of size cond(C~_t), the sums it is
// applied to cancel, and B~ - E~ C~^-1 E~^T cancels again: in plain fp64 the reduced system carries errors of u cond(C~_t) that a solver
// which does not eliminate never sees.  So the inverse is kept as an unevaluated sum hi + lo, and the track sums it is
// applied to are accumulated in double-double.  (contract(off): under the device default, -ffp-contract=fast, a + p with p = x y would become
// fma(x, y, a) and the two-sums below would lose their error terms.)
__device__ __forceinline__ void ba6_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// (hi, lo) += a b: the product by fma (error-free), the sum by Knuth's two-sum
__device__ __forceinline__ void ba6_dd_mac(double a, double b, double& hi, double& lo) {
#pragma clang fp contract(off)
  const double p = a * b, pe = fma(a, b, -p);
  double sum, se;
  ba6_two_sum(hi, p, sum, se);
  hi = sum; lo += se + pe;
}
// (hi, lo) += a (bh + bl)
__device__ __forceinline__ void ba6_dd_mac2(double a, double bh, double bl, double& hi, double& lo) {
  ba6_dd_mac(a, bh, hi, lo);
  lo += a * bl;
}
__device__ __forceinline__ void ba6_dd_add(double& hi, double& lo, double ohi, double olo) {
#pragma clang fp contract(off)
  double sum, se;
  ba6_two_sum(hi, ohi, sum, se);
  lo = (lo + olo) + se;   // (symmetric in the two operands: both lanes of a butterfly pair get the same pair)
  hi = sum;
}
template <int G>
__device__ __forceinline__ void ba6_group_allsum_dd(double& hi, double& lo) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const double ohi = __shfl_xor(hi, off, G), olo = __shfl_xor(lo, off, G);
    ba6_dd_add(hi, lo, ohi, olo);
  }
}
// w = (Xh + Xl) (th + tl), rounded once: Ci holds the inverse as 9 + 9 doubles (row-major hi, then lo)
__device__ __forceinline__ void ba6_apply_inv_dd(const double* Ci, const double* th, const double* tl, double* w) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double hi = 0.0, lo = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ba6_dd_mac(Ci[3 * r + c], th[c], hi, lo);
      lo += Ci[3 * r + c] * tl[c] + Ci[9 + 3 * r + c] * th[c];
    }
    w[r] = hi + lo;
  }
}

// One Newton step X + X (I - M X) for the symmetric 3 x 3 M (00 01 02 11 12 22) and its approximate inverse X (full, row-major), the
// residual I - M X accumulated in double-double so that the step sees the residual and not its rounding.  corr == NULL: X is replaced by
// the step's result; else X stays and the correction X (I - M X) goes to corr, so that X + corr is the inverse as an unevaluated pair.
__device__ __forceinline__ void ba6_refine_inv3(const double* m, double* X, double* corr) {
  const double M9[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
  double R[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double hi = (r == c) ? -1.0 : 0.0, lo = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) ba6_dd_mac(M9[3 * r + k], X[3 * k + c], hi, lo);
      R[3 * r + c] = -(hi + lo);
    }
  double Y[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Y[3 * r + c] = X[3 * r] * R[c] + X[3 * r + 1] * R[3 + c] + X[3 * r + 2] * R[6 + c];
  // (the inverse of a symmetric matrix: the two triangles of the correction are averaged)
  Y[1] = Y[3] = 0.5 * (Y[1] + Y[3]); Y[2] = Y[6] = 0.5 * (Y[2] + Y[6]); Y[5] = Y[7] = 0.5 * (Y[5] + Y[7]);
#pragma unroll
  for (int k = 0; k < 9; ++k) { if (corr) corr[k] = Y[k]; else X[k] += Y[k]; }
}
// A point whose damped block is badly conditioned -- max |C~| max |C~^-1| above GSFM_BA_DD_COND, as it is for a block that lost rank beyond
// the Tukey cut and is held up by the damping alone -- is "flagged": k_ba_prep_points refines its inverse to a pair (Cinv: the refined X,
// Cfix[0..8]: the correction, Cfix[9] = 1) and k_ba_point_pass / k_ba_cam_precond run its sums in double-double, as full_ba_kernels.hpp does for
// every point (DESIGN.md sections 16, 17).  Every other point keeps the plain fp64 path and its bytes.
#define GSFM_BA_DD_COND 1e5
#define GSFM_BA_FIX_DOUBLES 10
__device__ __forceinline__ void ba_pair(const double* Ci, const double* fix, double* X18) {
#pragma unroll
  for (int c = 0; c < 9; ++c) { X18[c] = Ci[c]; X18[9 + c] = fix[c]; }
}

// ---- point side ------------------------------------------------------------------------------------------------------------------
// Linearisation at x: per observation H_e and a_e (stored in track order), per point C_t = sum H_e into Dg and g_t = sum a_e into g.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba_lin_tracks(BaDev a, BaSlots sl, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t node = (size_t)a.n_cams + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const uint32_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_TRI_CAM_DOUBLES * c;
    double h[6] = {0, 0, 0, 0, 0, 0}, av[3] = {0, 0, 0};
    if (used_t && cam[15] != 0.0) {
      double J0[3], J1[3], r0, r1, rho0;
      reproj_corrected(cam, a.obs_xy[e], X[0] - x[3 * (size_t)c], X[1] - x[3 * (size_t)c + 1], X[2] - x[3 * (size_t)c + 2], a.leaf, J0, J1, r0, r1, rho0);
      h[0] = J0[0] * J0[0] + J1[0] * J1[0]; h[1] = J0[0] * J0[1] + J1[0] * J1[1]; h[2] = J0[0] * J0[2] + J1[0] * J1[2];
      h[3] = J0[1] * J0[1] + J1[1] * J1[1]; h[4] = J0[1] * J0[2] + J1[1] * J1[2]; h[5] = J0[2] * J0[2] + J1[2] * J1[2];
      av[0] = J0[0] * r0 + J1[0] * r1; av[1] = J0[1] * r0 + J1[1] * r1; av[2] = J0[2] * r0 + J1[2] * r1;
#pragma unroll
      for (int j = 0; j < 6; ++j) s[j] += h[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) s[6 + j] += av[j];
    }
    ba_store_h(a.Ht, e, h);
    a.At[3 * e] = av[0]; a.At[3 * e + 1] = av[1]; a.At[3 * e + 2] = av[2];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) s[j] = tri_group_allsum<G>(s[j]);
  if (tk.live && l == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) Dg[6 * node + j] = s[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[3 * node + j] = s[6 + j];
  }
}

// Cost at x: cost_t[t] = sum over the track's used observations of rho(|r|^2) / 2 (0 for a track without one).  r_out (n_obs x 2) and
// rho_out (n_obs), for gsfm_ba_residuals, may be NULL; an unused observation gets zeros.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba_cost_tracks(BaDev a, BaSlots sl, const double* __restrict__ x, double* __restrict__ cost_t,
                                                          double* __restrict__ r_out, double* __restrict__ rho_out) {
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t node = (size_t)a.n_cams + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const uint32_t c = a.obs_cam[e];
    const double* cam = a.cams + (size_t)GSFM_TRI_CAM_DOUBLES * c;
    double ex = 0.0, ey = 0.0, rho = 0.0;
    if (used_t && cam[15] != 0.0) {
      reproj_residual(cam, a.obs_xy[e], X[0] - x[3 * (size_t)c], X[1] - x[3 * (size_t)c + 1], X[2] - x[3 * (size_t)c + 2], ex, ey);
      rho = loss_leaf_simple(a.leaf, ex * ex + ey * ey).r0;
      acc += 0.5 * rho;
    }
    if (r_out) { r_out[2 * e] = ex; r_out[2 * e + 1] = ey; }
    if (rho_out) rho_out[e] = rho;
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) cost_t[tk.t] = acc;
}

// The point pass of the Schur product and the back-substitution:  u_t = Cinv_t (S_t sum_{e in t} H_e q_{k(e)} + add_t), with q = S v on the
// cameras (0 on inactive ones), add = the node vector b or NULL.  scaled_out: out_t = S_t u_t (the z_t the camera pass gathers), else u_t.
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba_point_pass(BaDev a, BaSlots sl, const double* __restrict__ q, const double* __restrict__ S,
                                                         const double* __restrict__ Cinv, const double* __restrict__ Cfix, const double* __restrict__ add,
                                                         double* __restrict__ out, int scaled_out) {
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  if (tk.live && Cfix[GSFM_BA_FIX_DOUBLES * (size_t)tk.t + 9] != 0.0) {   // a flagged point (the whole group): the sums and the inverse as pairs
    double yh[3] = {0.0, 0.0, 0.0}, yl[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = l; k < tk.len; k += G) {
      const size_t e = tk.ob + k;
      const size_t c = a.obs_cam[e];
      double h[6];
      ba_load_h(a.Ht, e, h);
      const double H9[9] = {h[0], h[1], h[2], h[1], h[3], h[4], h[2], h[4], h[5]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int i = 0; i < 3; ++i) ba6_dd_mac(H9[3 * r + i], q[3 * c + i], yh[r], yl[r]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ba6_group_allsum_dd<G>(yh[i], yl[i]);
    if (l == 0) {
      const size_t node = (size_t)a.n_cams + tk.t;
      const double sc[3] = {S[3 * node], S[3 * node + 1], S[3 * node + 2]};
      double th[3], tl[3], u[3], X18[18];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double hi = 0.0, lo = 0.0;
        ba6_dd_mac2(sc[i], yh[i], yl[i], hi, lo);
        if (add) ba6_dd_add(hi, lo, add[3 * node + i], 0.0);
        th[i] = hi; tl[i] = lo;
      }
      ba_pair(Cinv + 9 * (size_t)tk.t, Cfix + GSFM_BA_FIX_DOUBLES * (size_t)tk.t, X18);
      ba6_apply_inv_dd(X18, th, tl, u);
      double* o = out + 3 * (size_t)tk.t;
      o[0] = scaled_out ? sc[0] * u[0] : u[0]; o[1] = scaled_out ? sc[1] * u[1] : u[1]; o[2] = scaled_out ? sc[2] * u[2] : u[2];
    }
    return;
  }
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double h[6];
    ba_load_h(a.Ht, e, h);
    ba_sym_mac(h, q[3 * c], q[3 * c + 1], q[3 * c + 2], y0, y1, y2);
  }
  y0 = tri_group_allsum<G>(y0); y1 = tri_group_allsum<G>(y1); y2 = tri_group_allsum<G>(y2);
  if (tk.live && l == 0) {
    const size_t node = (size_t)a.n_cams + tk.t;
    const double s0 = S[3 * node], s1 = S[3 * node + 1], s2 = S[3 * node + 2];
    double t0 = s0 * y0, t1 = s1 * y1, t2 = s2 * y2;
    if (add) { t0 += add[3 * node]; t1 += add[3 * node + 1]; t2 += add[3 * node + 2]; }
    const double* Ci = Cinv + 9 * (size_t)tk.t;
    const double u0 = Ci[0] * t0 + Ci[1] * t1 + Ci[2] * t2, u1 = Ci[3] * t0 + Ci[4] * t1 + Ci[5] * t2, u2 = Ci[6] * t0 + Ci[7] * t1 + Ci[8] * t2;
    double* o = out + 3 * (size_t)tk.t;
    o[0] = scaled_out ? s0 * u0 : u0; o[1] = scaled_out ? s1 * u1 : u1; o[2] = scaled_out ? s2 * u2 : u2;
  }
}

// quad_t[t] = sum_{e in t} d^T H_e d with d = delta_t - delta_{k(e)}: the track's part of delta^T (J~^T J~) delta
template <int G>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_ba_quad_tracks(BaDev a, BaSlots sl, const double* __restrict__ delta, double* __restrict__ quad_t) {
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t node = (size_t)a.n_cams + tk.t;
  double d[3] = {0.0, 0.0, 0.0};
  if (tk.live) { d[0] = delta[3 * node]; d[1] = delta[3 * node + 1]; d[2] = delta[3 * node + 2]; }
  double acc = 0.0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double h[6];
    ba_load_h(a.Ht, e, h);
    const double v0 = d[0] - delta[3 * c], v1 = d[1] - delta[3 * c + 1], v2 = d[2] - delta[3 * c + 2];
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    ba_sym_mac(h, v0, v1, v2, y0, y1, y2);
    acc += v0 * y0 + v1 * y1 + v2 * y2;
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) quad_t[tk.t] = acc;
}

// ---- camera side: one wavefront per row -------------------------------------------------------------------------------------------
// The camera half of the linearisation: the row's blocks copied into camera order, g_k = -sum a_e and B_k = sum H_e.
__global__ void __launch_bounds__(256) k_ba_cam_lin(BaDev a, double* __restrict__ g, double* __restrict__ Dg) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t e = a.cobs[d];
    double h[6];
    ba_load_h(a.Ht, e, h);
    ba_store_h(a.Hc, d, h);
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] -= a.At[3 * e + j];
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[3 + j] += h[j];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
    for (int j = 0; j < 3; ++j) g[3 * (size_t)row + j] = acc[j];
    for (int j = 0; j < 6; ++j) Dg[6 * (size_t)row + j] = acc[3 + j];
  }
}

// The camera pass:  out_k = S_k sum_{e in k} H_e (q_k - z_{t(e)}) + D2_k p_k + add_k  on active rows (q, p, add may be NULL: zero).
// Inactive rows: p_k when identity_inactive (the PCG operator is the identity there), else 0.
//   Schur product   q = S p, z from the point pass:  out = S p
//   reduced rhs     q = NULL, z = -S C~^-1 b_p, add = b:  out = b_c - E~ C~^-1 b_p
__global__ void __launch_bounds__(256) k_ba_cam_pass(BaDev a, const double* __restrict__ q, const double* __restrict__ z, const double* __restrict__ p,
                                                      const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ add,
                                                      double* __restrict__ out, int identity_inactive) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t k3 = 3 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 3) out[k3 + lane] = (identity_inactive && p) ? p[k3 + lane] : 0.0;
    return;
  }
  double q0 = 0.0, q1 = 0.0, q2 = 0.0;
  if (q) { q0 = q[k3]; q1 = q[k3 + 1]; q2 = q[k3 + 2]; }
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    const size_t t = a.ctrk[d];
    double h[6];
    ba_load_h(a.Hc, d, h);
    ba_sym_mac(h, q0 - z[3 * t], q1 - z[3 * t + 1], q2 - z[3 * t + 2], y0, y1, y2);
  }
  y0 = wave_sum(y0); y1 = wave_sum(y1); y2 = wave_sum(y2);
  if (lane == 0) {
    const double y[3] = {y0, y1, y2};
    for (int c = 0; c < 3; ++c) {
      double o = S[k3 + c] * y[c];
      if (p) o += D2[k3 + c] * p[k3 + c];
      if (add) o += add[k3 + c];
      out[k3 + c] = o;
    }
  }
}

// The preconditioner, the block diagonal of the Schur complement (Ceres' SCHUR_JACOBI), inverted per camera:
//   M_k = S_k (sum_{e in k} H_e - H_e G_t H_e) S_k + D2_k,   G_t = S_t C~_t^-1 S_t;   the identity on inactive rows.
__global__ void __launch_bounds__(256) k_ba_cam_precond(BaDev a, const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ Gt,
                                                         const double* __restrict__ Cinv, const double* __restrict__ Cfix, double* __restrict__ Minv) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  double* Mi = Minv + 9 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 9) Mi[lane] = (lane % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  double acc[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t end = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < end; d += 64) {
    double h[6], gt[6];
    ba_load_h(a.Hc, d, h);
    ba_load_h(Gt, a.ctrk[d], gt);
    const double H9[9] = {h[0], h[1], h[2], h[1], h[3], h[4], h[2], h[4], h[5]};
    const size_t tt = a.ctrk[d];
    if (Cfix[GSFM_BA_FIX_DOUBLES * tt + 9] != 0.0) {   // a flagged point: H - H S C~^-1 S H cancels to the damping's size; column by column through the pair
      const size_t node = (size_t)a.n_cams + tt;
      const double sc[3] = {S[3 * node], S[3 * node + 1], S[3 * node + 2]}, zl[3] = {0.0, 0.0, 0.0};
      double X18[18], U[9];   // U = S C~^-1 S H
      ba_pair(Cinv + 9 * tt, Cfix + GSFM_BA_FIX_DOUBLES * tt, X18);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double tc[3] = {sc[0] * H9[c], sc[1] * H9[3 + c], sc[2] * H9[6 + c]};
        double x[3];
        ba6_apply_inv_dd(X18, tc, zl, x);
        U[c] = sc[0] * x[0]; U[3 + c] = sc[1] * x[1]; U[6 + c] = sc[2] * x[2];
      }
      const int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double hi = H9[3 * rr[j] + cc[j]], lo = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) ba6_dd_mac(-H9[3 * rr[j] + k], U[3 * k + cc[j]], hi, lo);
        acc[j] += hi + lo;
      }
      continue;
    }
    double W[9];   // W = G H
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double w0 = 0.0, w1 = 0.0, w2 = 0.0;
      ba_sym_mac(gt, H9[c], H9[3 + c], H9[6 + c], w0, w1, w2);
      W[c] = w0; W[3 + c] = w1; W[6 + c] = w2;
    }
    // H W, upper triangle
    acc[0] += h[0] - (H9[0] * W[0] + H9[1] * W[3] + H9[2] * W[6]);
    acc[1] += h[1] - (H9[0] * W[1] + H9[1] * W[4] + H9[2] * W[7]);
    acc[2] += h[2] - (H9[0] * W[2] + H9[1] * W[5] + H9[2] * W[8]);
    acc[3] += h[3] - (H9[3] * W[1] + H9[4] * W[4] + H9[5] * W[7]);
    acc[4] += h[4] - (H9[3] * W[2] + H9[4] * W[5] + H9[5] * W[8]);
    acc[5] += h[5] - (H9[6] * W[2] + H9[7] * W[5] + H9[8] * W[8]);
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
    const size_t k3 = 3 * (size_t)row;
    const double s0 = S[k3], s1 = S[k3 + 1], s2 = S[k3 + 2];
    const double M[6] = {s0 * acc[0] * s0 + D2[k3], s0 * acc[1] * s1, s0 * acc[2] * s2, s1 * acc[3] * s1 + D2[k3 + 1], s1 * acc[4] * s2, s2 * acc[5] * s2 + D2[k3 + 2]};
    double inv[9];
    pos_inv3(M, inv);
    for (int j = 0; j < 9; ++j) Mi[j] = inv[j];
  }
}

// ---- per-node and per-point vector kernels ----------------------------------------------------------------------------------------
// Start of a step, every node: D^2 = clamp(S^2 diag) / radius (LevenbergMarquardtStrategy) and b = S g; zero on inactive nodes.
__global__ void k_ba_prep_nodes(size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ Dg, const double* __restrict__ g,
                                const double* __restrict__ S, double radius, double min_diag, double max_diag, double* __restrict__ D2, double* __restrict__ b) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_nodes) return;
  const double* D = Dg + 6 * k;
  const double dg[3] = {D[0], D[3], D[5]};
  for (int c = 0; c < 3; ++c) {
    const double s = S[3 * k + c];
    D2[3 * k + c] = active[k] ? fmin(fmax(s * s * dg[c], min_diag), max_diag) / radius : 0.0;
    b[3 * k + c] = active[k] ? s * g[3 * k + c] : 0.0;
  }
}
// ... every point: C~_t = S_t C_t S_t + D2_t inverted by cofactors (positive definite by the diagonal clamp), G_t = S_t C~^-1 S_t for the
// preconditioner and zneg_t = -S_t C~^-1 b_t for the reduced right-hand side; zeros on inactive points.
__global__ void k_ba_prep_points(uint32_t n_cams, uint32_t n_tracks, const uint8_t* __restrict__ active, const double* __restrict__ Dg,
                                 const double* __restrict__ S, const double* __restrict__ D2, const double* __restrict__ b, double* __restrict__ Cinv,
                                 double* __restrict__ Cfix, double* __restrict__ Gt, double* __restrict__ zneg) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tracks) return;
  const size_t node = (size_t)n_cams + t;
  double Ci[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, G6[6] = {0, 0, 0, 0, 0, 0}, zn[3] = {0, 0, 0}, fix[GSFM_BA_FIX_DOUBLES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (active[node]) {
    const double* D = Dg + 6 * node;
    const double s0 = S[3 * node], s1 = S[3 * node + 1], s2 = S[3 * node + 2];
    const double M[6] = {s0 * D[0] * s0 + D2[3 * node], s0 * D[1] * s1, s0 * D[2] * s2, s1 * D[3] * s1 + D2[3 * node + 1], s1 * D[4] * s2,
                         s2 * D[5] * s2 + D2[3 * node + 2]};
    pos_inv3(M, Ci);
    double mm = 0.0, mi = 0.0;
    for (int c = 0; c < 6; ++c) mm = fmax(mm, fabs(M[c]));
    for (int c = 0; c < 9; ++c) mi = fmax(mi, fabs(Ci[c]));
    const bool flagged = !(mm * mi <= GSFM_BA_DD_COND);   // (a NaN is flagged too)
    if (flagged) {
      ba6_refine_inv3(M, Ci, nullptr);
      ba6_refine_inv3(M, Ci, nullptr);
      ba6_refine_inv3(M, Ci, fix);   // C~^-1 = Ci + fix[0..8] to about u^2
      fix[9] = 1.0;
    }
    G6[0] = s0 * Ci[0] * s0; G6[1] = s0 * Ci[1] * s1; G6[2] = s0 * Ci[2] * s2; G6[3] = s1 * Ci[4] * s1; G6[4] = s1 * Ci[5] * s2; G6[5] = s2 * Ci[8] * s2;
    const double b0 = b[3 * node], b1 = b[3 * node + 1], b2 = b[3 * node + 2];
    if (flagged) {
      const double bh[3] = {b0, b1, b2}, bl[3] = {0.0, 0.0, 0.0};
      double X18[18], w[3];
      ba_pair(Ci, fix, X18);
      ba6_apply_inv_dd(X18, bh, bl, w);
      zn[0] = -s0 * w[0]; zn[1] = -s1 * w[1]; zn[2] = -s2 * w[2];
    } else {
      zn[0] = -s0 * (Ci[0] * b0 + Ci[1] * b1 + Ci[2] * b2);
      zn[1] = -s1 * (Ci[3] * b0 + Ci[4] * b1 + Ci[5] * b2);
      zn[2] = -s2 * (Ci[6] * b0 + Ci[7] * b1 + Ci[8] * b2);
    }
  }
  for (int c = 0; c < GSFM_BA_FIX_DOUBLES; ++c) Cfix[GSFM_BA_FIX_DOUBLES * t + c] = fix[c];
  for (int c = 0; c < 9; ++c) Cinv[9 * t + c] = Ci[c];
  for (int c = 0; c < 6; ++c) Gt[6 * t + c] = G6[c];
  for (int c = 0; c < 3; ++c) zneg[3 * t + c] = zn[c];
}
// PCG start on the cameras: y = 0, r = rhs, z = M^-1 r, p = z, q = S p (0 on inactive rows)
__global__ void k_ba_pcg_init(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ rhs, const double* __restrict__ Minv,
                              const double* __restrict__ S, double* __restrict__ y, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                              double* __restrict__ q) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams) return;
  const size_t k3 = 3 * (size_t)k;
  const double* Mi = Minv + 9 * (size_t)k;
  const double r0 = rhs[k3], r1 = rhs[k3 + 1], r2 = rhs[k3 + 2];
  for (int c = 0; c < 3; ++c) {
    const double zc = Mi[3 * c] * r0 + Mi[3 * c + 1] * r1 + Mi[3 * c + 2] * r2;
    y[k3 + c] = 0.0; r[k3 + c] = rhs[k3 + c]; z[k3 + c] = zc; p[k3 + c] = zc;
    q[k3 + c] = active[k] ? S[k3 + c] * zc : 0.0;
  }
}
// out = sign S v on active nodes, 0 elsewhere (q = S y for the back-substitution, delta = -S y for the step)
__global__ void k_ba_scale(size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ S, const double* __restrict__ v, double sign,
                           double* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_nodes) return;
  for (int c = 0; c < 3; ++c) out[3 * k + c] = active[k] ? sign * S[3 * k + c] * v[3 * k + c] : 0.0;
}

// ---- reductions over the nodes (GSFM_POS_PARTS partials, then k_pos_reduce) --------------------------------------------------------
__global__ void __launch_bounds__(256) k_ba_sum(const double* __restrict__ a, size_t n, double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)GSFM_POS_PARTS * 256) acc += a[i];
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// the sum of the active nodes' coordinate `axis` of a
__global__ void __launch_bounds__(256) k_ba_axis_sum(const double* __restrict__ a, const uint8_t* __restrict__ active, size_t n_nodes, int axis,
                                                      double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_nodes; i += (size_t)GSFM_POS_PARTS * 256)
    if (active[i]) acc += a[3 * i + axis];
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// The gauge, first half: delta loses its mean over the active nodes per axis, and v = x - mean(x) is the scaling direction about the
// centroid (0 on inactive nodes).  scal[s_d .. s_d + 2] and scal[s_x .. s_x + 2] hold the axis sums; inv_count = 1 / (active nodes).
__global__ void k_ba_center(size_t n_nodes, const uint8_t* __restrict__ active, const double* __restrict__ scal, int s_d, int s_x, double inv_count,
                            const double* __restrict__ x, double* __restrict__ delta, double* __restrict__ v) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_nodes) return;
  for (int c = 0; c < 3; ++c) {
    delta[3 * k + c] = active[k] ? delta[3 * k + c] - scal[s_d + c] * inv_count : 0.0;
    v[3 * k + c] = active[k] ? x[3 * k + c] - scal[s_x + c] * inv_count : 0.0;
  }
}

}  // namespace gsfm
