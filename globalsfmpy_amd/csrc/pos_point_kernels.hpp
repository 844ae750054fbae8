// Device kernels of camera-position estimation with point-to-camera constraints (include/gsfm_posp.h): the position problem of
// pos_kernels.hpp plus, per used observation o of camera k and point t, Theia's PairwiseTranslationError between the camera centre and the
// point, r_o = w_p ((X_t - c_k) / n - ray_o).
//
// Structure.  With w = X_t - c_k the point Jacobian of an observation is A = w_p (I - u u^T) / n and the camera Jacobian is -A, so with
// H_o = A~^T A~ and a_o = A~^T r~ (A~, r~ after Ceres' Corrector) the camera-point part of the normal matrix has ba_kernels.hpp's block
// structure -- B_k = sum H_o, C_t = sum H_o, off-diagonal -H_o, g_k = -sum a_o, g_t = +sum a_o -- and the camera-camera part is
// pos_kernels.hpp's edge Laplacian.  Both are kept UNSCALED in the layouts of those files (H per directed edge entry; Ht / At per
// observation in track order, Hc in camera order), so the point pass, the quadratic form over tracks, the points' inverses and every
// vector kernel are theirs, called as they are.  New here: the rays, the track side of the linearisation and of the cost for a 3-vector
// direction residual, and the three camera-row kernels that carry the edge entries and the observation blocks of a row together.
//
// Order of the sums: a track's lane group (G = 4 / 16 / 64, xor butterfly); a camera row's wavefront strides first the row's edge entries,
// then its used observations in ascending observation index, then the fixed shuffle tree.  Every loop is bounded by a CSR length known at
// launch, every shuffle is executed by all lanes of its wavefront, and there are no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pos_kernels.hpp"
#include "ba_kernels.hpp"

namespace gsfm {

// what the observation side needs beside BaDev (whose cams, obs_xy and leaf are not read here)
struct PpObs {
  const uint8_t* cam_used;   // N: the camera appears in an edge (the fixed camera included)
  const double* ray;         // n_obs x 3: unit rays in the world frame (k_pp_rays; zero for an observation that is not used)
  double w;                  // point_to_camera_weight
  const DevLoss* loss;       // the problem's loss, as PosDev's
};

// ray_o = normalise(R(aa_k)^T ((x - u) / f, (y - v) / f, 1)): one lane per observation, zeros when the observation is not used
__global__ void __launch_bounds__(256) k_pp_rays(uint64_t n_obs, const uint32_t* __restrict__ obs_cam, const double2* __restrict__ obs_xy,
                                                 const uint8_t* __restrict__ obs_used, const double* __restrict__ ray_rot_aa,
                                                 const double* __restrict__ intrinsics, double* __restrict__ ray) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_obs) return;
  double d[3] = {0.0, 0.0, 0.0};
  if (obs_used[e]) {
    const size_t c = obs_cam[e];
    const double f = intrinsics[3 * c], u = intrinsics[3 * c + 1], v = intrinsics[3 * c + 2];
    const double2 xy = obs_xy[e];
    const double t[3] = {(xy.x - u) / f, (xy.y - v) / f, 1.0};
    pos_world_direction(ray_rot_aa + 3 * c, t, d);
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] /= n; d[1] /= n; d[2] /= n;
  }
  ray[3 * e] = d[0]; ray[3 * e + 1] = d[1]; ray[3 * e + 2] = d[2];
}

// The corrected Jacobian A~ (row-major 3 x 3, with respect to the far end m of w = c_m - c_k) and the corrected residual r~ of a direction
// residual r = weight (w / n - d): k_pos_lin's arithmetic with the weight applied to r and to A before the loss sees s = |r|^2
template <int LM>
__device__ __forceinline__ void pp_direction_lin(double w0, double w1, double w2, const double* d, double weight, const DevLoss* __restrict__ loss,
                                                 double* A, double* rt) {
  double r[3], u[3], n;
  const bool unit = pos_residual(w0, w1, w2, d, r, u, n);
  r[0] *= weight; r[1] *= weight; r[2] *= weight;
  const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const Rho3 rho = loss_eval<LM>(loss, s);
  const Corrector c = make_corrector(s, rho);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[3 * i + j] = weight * (unit ? ((i == j ? 1.0 : 0.0) - u[i] * u[j]) / n : (i == j ? 1.0 : 0.0));
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
  rt[0] = c.residual_scaling * r[0]; rt[1] = c.residual_scaling * r[1]; rt[2] = c.residual_scaling * r[2];
}
__device__ __forceinline__ void pp_gram(const double* A, double* h) {
  h[0] = A[0] * A[0] + A[3] * A[3] + A[6] * A[6];
  h[1] = A[0] * A[1] + A[3] * A[4] + A[6] * A[7];
  h[2] = A[0] * A[2] + A[3] * A[5] + A[6] * A[8];
  h[3] = A[1] * A[1] + A[4] * A[4] + A[7] * A[7];
  h[4] = A[1] * A[2] + A[4] * A[5] + A[7] * A[8];
  h[5] = A[2] * A[2] + A[5] * A[5] + A[8] * A[8];
}

// ---- track side ---------------------------------------------------------------------------------------------------------------------
// Linearisation at x: per observation H_o and a_o (ba_kernels.hpp's Ht / At, zero for an observation that is not used), per point
// C_t = sum H_o into Dg and g_t = sum a_o into g.
template <int G, int LM>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_pp_lin_tracks(BaDev a, BaSlots sl, PpObs p, const double* __restrict__ x, double* __restrict__ g,
                                                         double* __restrict__ Dg) {
  const BaTrack tk = ba_track<G>(a, sl);
  const int l = threadIdx.x % G;
  const size_t node = (size_t)a.n_cams + tk.t;
  const bool used_t = tk.live && a.track_used[tk.t] != 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (used_t) { X[0] = x[3 * node]; X[1] = x[3 * node + 1]; X[2] = x[3 * node + 2]; }
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = l; k < tk.len; k += G) {
    const size_t e = tk.ob + k;
    const size_t c = a.obs_cam[e];
    double h[6] = {0, 0, 0, 0, 0, 0}, av[3] = {0, 0, 0};
    if (used_t && p.cam_used[c] != 0) {
      double A[9], rt[3];
      pp_direction_lin<LM>(X[0] - x[3 * c], X[1] - x[3 * c + 1], X[2] - x[3 * c + 2], p.ray + 3 * e, p.w, p.loss, A, rt);
      pp_gram(A, h);
#pragma unroll
      for (int col = 0; col < 3; ++col) av[col] = A[col] * rt[0] + A[3 + col] * rt[1] + A[6 + col] * rt[2];
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

// Cost at x: cost_t[t] = sum over the track's used observations of rho(|r_o|^2) / 2.  r_out (n_obs x 3, the weighted residual) and rho_out
// (n_obs) may be NULL; an observation that is not used gets zeros.
template <int G, int LM>
__global__ void GSFM_BA_TRACK_BOUNDS(G) k_pp_cost_tracks(BaDev a, BaSlots sl, PpObs p, const double* __restrict__ x, double* __restrict__ cost_t,
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
    const size_t c = a.obs_cam[e];
    double r[3] = {0.0, 0.0, 0.0}, rho = 0.0;
    if (used_t && p.cam_used[c] != 0) {
      double u[3], n;
      pos_residual(X[0] - x[3 * c], X[1] - x[3 * c + 1], X[2] - x[3 * c + 2], p.ray + 3 * e, r, u, n);
      r[0] *= p.w; r[1] *= p.w; r[2] *= p.w;
      rho = loss_value<LM>(p.loss, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      acc += 0.5 * rho;
    }
    if (r_out) { r_out[3 * e] = r[0]; r_out[3 * e + 1] = r[1]; r_out[3 * e + 2] = r[2]; }
    if (rho_out) rho_out[e] = rho;
  }
  acc = tri_group_allsum<G>(acc);
  if (tk.live && l == 0) cost_t[tk.t] = acc;
}

// ---- camera side: one wavefront per row, the edge entries and then the observations ------------------------------------------------------
// The camera rows of the linearisation: what k_pos_lin does on the row's edge entries (H per entry stored, g_k -= A~^T r~, D_k += H) and what
// k_ba_cam_lin does on its observations (Ht copied into camera order, g_k -= a_o, D_k += H_o), one reduction, one write of g_k and Dg_k.
template <int LM>
__global__ void __launch_bounds__(256) k_pp_cam_lin(PosDev ed, BaDev a, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ Dg) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;   // (wave-uniform)
  const double xk0 = x[3 * (size_t)row], xk1 = x[3 * (size_t)row + 1], xk2 = x[3 * (size_t)row + 2];
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t eend = ed.row_ptr[row + 1];
  for (uint32_t d = ed.row_ptr[row] + lane; d < eend; d += 64) {
    const uint32_t m = ed.nbr[d];
    double A[9], rt[3], h[6];
    pp_direction_lin<LM>(x[3 * (size_t)m] - xk0, x[3 * (size_t)m + 1] - xk1, x[3 * (size_t)m + 2] - xk2, ed.dir_k + 3 * (size_t)d, 1.0, ed.loss, A, rt);
#pragma unroll
    for (int col = 0; col < 3; ++col) acc[col] -= A[col] * rt[0] + A[3 + col] * rt[1] + A[6 + col] * rt[2];
    pp_gram(A, h);
    ba_store_h(ed.H, d, h);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[3 + k] += h[k];
  }
  const uint32_t oend = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < oend; d += 64) {
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
  for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    for (int k = 0; k < 3; ++k) g[3 * (size_t)row + k] = acc[k];
    for (int k = 0; k < 6; ++k) Dg[6 * (size_t)row + k] = acc[3 + k];
  }
}

// The camera pass:  out_k = S_k [ sum_edges H_e (q_k - q_m) + sum_obs H_o (q_k - z_t) ] + D2_k p_k + add_k  on active rows (q, p, add may be
// NULL: zero; without q the edge entries contribute nothing and are not read).  Inactive rows: p_k when identity_inactive, else 0.
//   Schur product   q = S p, z from the point pass
//   reduced rhs     q = NULL, z = -S C~^-1 b_p, add = b
__global__ void __launch_bounds__(256) k_pp_cam_pass(PosDev ed, BaDev a, const double* __restrict__ q, const double* __restrict__ z,
                                                      const double* __restrict__ p, const double* __restrict__ S, const double* __restrict__ D2,
                                                      const double* __restrict__ add, double* __restrict__ out, int identity_inactive) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  const size_t k3 = 3 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 3) out[k3 + lane] = (identity_inactive && p) ? p[k3 + lane] : 0.0;
    return;
  }
  double q0 = 0.0, q1 = 0.0, q2 = 0.0;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  if (q) {
    q0 = q[k3]; q1 = q[k3 + 1]; q2 = q[k3 + 2];
    const uint32_t eend = ed.row_ptr[row + 1];
    for (uint32_t d = ed.row_ptr[row] + lane; d < eend; d += 64) {
      const size_t m = ed.nbr[d];
      double h[6];
      ba_load_h(ed.H, d, h);
      ba_sym_mac(h, q0 - q[3 * m], q1 - q[3 * m + 1], q2 - q[3 * m + 2], y0, y1, y2);
    }
  }
  const uint32_t oend = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < oend; d += 64) {
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

// The preconditioner, the block diagonal of the reduced operator, inverted per camera:
//   M_k = S_k (sum_edges H_e + sum_obs (H_o - H_o G_t H_o)) S_k + D2_k,   G_t = S_t C~_t^-1 S_t;   the identity on inactive rows.
// An observation of a flagged point (ba_kernels.hpp: GSFM_BA_DD_COND) takes k_ba_cam_precond's path through the inverse's pair.
__global__ void __launch_bounds__(256) k_pp_cam_precond(PosDev ed, BaDev a, const double* __restrict__ S, const double* __restrict__ D2,
                                                         const double* __restrict__ Gt, const double* __restrict__ Cinv, const double* __restrict__ Cfix,
                                                         double* __restrict__ Minv) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.n_cams) return;
  double* Mi = Minv + 9 * (size_t)row;
  if (!a.active[row]) {
    if (lane < 9) Mi[lane] = (lane % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  double acc[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t eend = ed.row_ptr[row + 1];
  for (uint32_t d = ed.row_ptr[row] + lane; d < eend; d += 64) {
    double h[6];
    ba_load_h(ed.H, d, h);
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] += h[j];
  }
  const uint32_t oend = a.crow_ptr[row + 1];
  for (uint32_t d = a.crow_ptr[row] + lane; d < oend; d += 64) {
    double h[6], gt[6];
    const size_t tt = a.ctrk[d];
    ba_load_h(a.Hc, d, h);
    ba_load_h(Gt, tt, gt);
    const double H9[9] = {h[0], h[1], h[2], h[1], h[3], h[4], h[2], h[4], h[5]};
    if (Cfix[GSFM_BA_FIX_DOUBLES * tt + 9] != 0.0) {   // a flagged point: H - H S C~^-1 S H cancels to the damping's size; column by column through the pair
      const size_t node = (size_t)a.n_cams + tt;
      const double sc[3] = {S[3 * node], S[3 * node + 1], S[3 * node + 2]}, zl[3] = {0.0, 0.0, 0.0};
      double X18[18], U[9];   // U = S C~^-1 S H
      ba_pair(Cinv + 9 * tt, Cfix + GSFM_BA_FIX_DOUBLES * tt, X18);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double tc[3] = {sc[0] * H9[c], sc[1] * H9[3 + c], sc[2] * H9[6 + c]};
        double xx[3];
        ba6_apply_inv_dd(X18, tc, zl, xx);
        U[c] = sc[0] * xx[0]; U[3 + c] = sc[1] * xx[1]; U[6 + c] = sc[2] * xx[2];
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

// scal[out] = scal[a] + scal[b] (the cost and the quadratic form are an edge sum plus a track sum)
__global__ void k_pp_add(double* __restrict__ scal, int a, int b, int out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[out] = scal[a] + scal[b];
}

}  // namespace gsfm
