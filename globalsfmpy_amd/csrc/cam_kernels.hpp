// K5: the one-lane-per-camera kernels -- k_cam_rotT, the quaternion cache, LM diagonal / preconditioner (k_cam_prep), the gauge
// projection, the step k_cam_step and the tangent maps.  Launched from solver_launch.hpp, solver_pcg.hpp and solver_lm.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"

namespace gsfm {

// u_k = R_k^T p_k (the PCG vector kernels produce it together with p; this is for the other callers of the mat-vec)
__device__ __forceinline__ void rot_transpose_apply(const Quat& q, const double* p, double* u) {
  double R[9];
  qmat(q, R);
  u[0] = R[0] * p[0] + R[3] * p[1] + R[6] * p[2];
  u[1] = R[1] * p[0] + R[4] * p[1] + R[7] * p[2];
  u[2] = R[2] * p[0] + R[5] * p[1] + R[8] * p[2];
}
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_rotT(const double* __restrict__ p, const double2* __restrict__ q, uint32_t n, double* __restrict__ u) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k >= n) return;
  const Quat qq{q[2 * (size_t)k].x, q[2 * (size_t)k].y, q[2 * (size_t)k + 1].x, q[2 * (size_t)k + 1].y};
  double v[3];
  rot_transpose_apply(qq, p + 3 * (size_t)k, v);
  u[3 * (size_t)k] = v[0]; u[3 * (size_t)k + 1] = v[1]; u[3 * (size_t)k + 2] = v[2];
}

// ------------------------------------------------------------------------------------------
// K5: camera kernels
// ------------------------------------------------------------------------------------------
// state -> quaternion cache.  param_dim 3: x = angle-axis; 4: x is already (x,y,z,w).
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_cache(const double* __restrict__ x, uint32_t n, int param_dim,
                                                          double2* __restrict__ q) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k >= n) return;
  Quat qq;
  if (param_dim == 3) qq = aa_to_quat(x[3 * (size_t)k], x[3 * (size_t)k + 1], x[3 * (size_t)k + 2]);
  else qq = Quat{x[4 * (size_t)k], x[4 * (size_t)k + 1], x[4 * (size_t)k + 2], x[4 * (size_t)k + 3]};
  q[2 * (size_t)k] = make_double2(qq.x, qq.y);
  q[2 * (size_t)k + 1] = make_double2(qq.z, qq.w);
}

// quaternion state -> angle-axis (ceres::QuaternionToAngleAxis), estimator.cpp:185-194
__global__ void __launch_bounds__(GSFM_BLOCK) k_quat_to_aa(const double* __restrict__ x, const double* __restrict__ active,
                                                           uint32_t n, double* __restrict__ aa) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k >= n) return;
  if (active[k] == 0.0) return;  // views never touched by an edge keep their input value
  const Quat q{x[4 * (size_t)k], x[4 * (size_t)k + 1], x[4 * (size_t)k + 2], x[4 * (size_t)k + 3]};
  double e[3], s, th;
  quat_log(q, e, &s, &th);
  aa[3 * (size_t)k] = e[0]; aa[3 * (size_t)k + 1] = e[1]; aa[3 * (size_t)k + 2] = e[2];
}

__device__ __forceinline__ void cam_tangent_maps(const double* __restrict__ x, size_t k, int param_dim, double* T, double* Tinv) {
  if (param_dim == 3) {
    const double w[3] = {x[3 * k], x[3 * k + 1], x[3 * k + 2]};
    jl_and_inverse(w, T, Tinv);
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) { T[c] = 0.0; Tinv[c] = 0.0; }
    T[0] = T[4] = T[8] = 2.0; Tinv[0] = Tinv[4] = Tinv[8] = 0.5;
  }
}

struct PrepArgs {
  uint32_t n;
  int param_dim;
  const double* x;
  const double* gD;       // 9 per camera (eta space)
  double* scale;          // 3 per camera: Jacobi column scaling, fixed at iteration 0
  int init_scale;         // 1 at iteration 0
  int jacobi_scaling;
  double radius, min_diag, max_diag;
  const double* radius_dev;  // non-null: the trust-region radius is read from here (device-side LM control) instead of `radius`
  double* Mblk;           // 6: D + Lambda
  double* Minv;           // 6
  double* Lam;            // 6: damping block in eta space
  double* Tinv;           // 9
  double* b;              // 3: -g_eta
  double* gmax_partials;  // [gridDim.x]
};
// LM diagonal (LevenbergMarquardtStrategy::ComputeStep), block-Jacobi preconditioner and the
// gradient max-norm ||x - Plus(x, -g)||_inf, all per camera.
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_prep(PrepArgs a) {
  __shared__ double lds[8];
  double gm = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    double T[9], Ti[9];
    cam_tangent_maps(a.x, k, a.param_dim, T, Ti);
    const double* gd = a.gD + 9 * (size_t)k;
    const double g[3] = {gd[0], gd[1], gd[2]};
    const double D[6] = {gd[3], gd[4], gd[5], gd[6], gd[7], gd[8]};
    // squared column norms in the reference's parameter space: diag(T^T D T)
    double dd[3], gdl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t0 = T[c], t1 = T[3 + c], t2 = T[6 + c];
      double v[3];
      const double tv[3] = {t0, t1, t2};
      sym3_mulvec(D, tv, v);
      dd[c] = t0 * v[0] + t1 * v[1] + t2 * v[2];
      gdl[c] = t0 * g[0] + t1 * g[1] + t2 * g[2];   // (T^T g)_c
    }
    double sc[3];
    if (a.init_scale) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { sc[c] = a.jacobi_scaling ? 1.0 / (1.0 + sqrt(dd[c])) : 1.0; a.scale[3 * (size_t)k + c] = sc[c]; }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) sc[c] = a.scale[3 * (size_t)k + c];
    }
    double lam[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double s2 = sc[c] * sc[c];
      lam[c] = fmin(fmax(s2 * dd[c], a.min_diag), a.max_diag) / ((a.radius_dev ? *a.radius_dev : a.radius) * s2);
    }
    // Lambda_eta = Tinv^T diag(lam) Tinv
    double L[6];
    L[0] = lam[0] * Ti[0] * Ti[0] + lam[1] * Ti[3] * Ti[3] + lam[2] * Ti[6] * Ti[6];
    L[1] = lam[0] * Ti[0] * Ti[1] + lam[1] * Ti[3] * Ti[4] + lam[2] * Ti[6] * Ti[7];
    L[2] = lam[0] * Ti[0] * Ti[2] + lam[1] * Ti[3] * Ti[5] + lam[2] * Ti[6] * Ti[8];
    L[3] = lam[0] * Ti[1] * Ti[1] + lam[1] * Ti[4] * Ti[4] + lam[2] * Ti[7] * Ti[7];
    L[4] = lam[0] * Ti[1] * Ti[2] + lam[1] * Ti[4] * Ti[5] + lam[2] * Ti[7] * Ti[8];
    L[5] = lam[0] * Ti[2] * Ti[2] + lam[1] * Ti[5] * Ti[5] + lam[2] * Ti[8] * Ti[8];
    double M[6], Mi[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { M[c] = D[c] + L[c]; a.Lam[6 * (size_t)k + c] = L[c]; a.Mblk[6 * (size_t)k + c] = M[c]; }
    sym3_inverse(M, Mi);
#pragma unroll
    for (int c = 0; c < 6; ++c) a.Minv[6 * (size_t)k + c] = Mi[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) a.Tinv[9 * (size_t)k + c] = Ti[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.b[3 * (size_t)k + c] = -g[c];
    if (a.param_dim == 3) gm = fmax(fabs(gdl[0]), fmax(fabs(gdl[1]), fabs(gdl[2])));
    else {
      // || x - Plus(x, -g) ||_inf with the quaternion Plus
      const double d0 = -gdl[0], d1 = -gdl[1], d2 = -gdl[2];
      const double nd = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      const Quat q{a.x[4 * (size_t)k], a.x[4 * (size_t)k + 1], a.x[4 * (size_t)k + 2], a.x[4 * (size_t)k + 3]};
      if (nd > 0.0) {
        double sn, cs;
        sincos(nd, &sn, &cs);
        const double kk = sn / nd;
        const Quat r = qmul(Quat{kk * d0, kk * d1, kk * d2, cs}, q);
        gm = fmax(fmax(fabs(q.x - r.x), fabs(q.y - r.y)), fmax(fabs(q.z - r.z), fabs(q.w - r.w)));
      }
    }
  }
  const double t = block_max_bcast(gm, lds);
  if (threadIdx.x == 0) a.gmax_partials[blockIdx.x] = t;
}
__global__ void __launch_bounds__(GSFM_BLOCK) k_max_partials(const double* __restrict__ partials, int n, double* out) {
  __shared__ double lds[8];
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += GSFM_BLOCK) v = fmax(v, partials[k]);
  const double t = block_max_bcast(v, lds);
  if (threadIdx.x == 0) out[0] = t;
}

// Absolute floor of the PCG tolerance (round 5).  A relative residual of 1e-12 stands in for the reference's exact Cholesky solve; on a step of
// 0.1 rad that is an error of 1e-13 rad, and that -- not twelve digits of a step that is itself 1e-9 rad long -- is what the answer can feel.  A
// solve therefore also stops once block-Jacobi's estimate of what ANY camera's step still lacks is below `floor` radians:
//   |delta_k|^2 = |Tinv_k Minv_k r_k|^2 <= |Tinv_k|^2 |Minv_k| (r_k . Minv_k r_k) <= B (r . Minv r),   B = max_k |Tinv_k|_F^2 |Minv_k|_F,
// i.e. once r.z <= floor^2 / B.  B is taken here, once per LM step (cameras without an edge excluded: their residual is zero); the init
// kernels of the solves turn it into a floor under the relative tolerance.  Decisive for disconnected problems (C4: thirteen scenes have
// converged to 1e-12 rad steps while the fourteenth iterates on -- each of their solves used to run 40 iterations on a right-hand side of nothing).
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_bound(const double* __restrict__ Minv, const double* __restrict__ Tinv, const double* __restrict__ active, uint32_t n, double* partials) {
  __shared__ double lds[8];
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  double v = 0.0;
  if (k < n && active[k] != 0.0) {
    const double* M = Minv + 6 * (size_t)k;
    const double* T = Tinv + 9 * (size_t)k;
    const double m2 = M[0] * M[0] + M[3] * M[3] + M[5] * M[5] + 2.0 * (M[1] * M[1] + M[2] * M[2] + M[4] * M[4]);
    double t2 = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) t2 += T[c] * T[c];
    v = t2 * sqrt(m2);
  }
  const double t = block_max_bcast(v, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// relative tolerance of a solve whose initial r.z is rz0: the requested one, or the one the absolute floor allows
__device__ __forceinline__ double cg_tol_with_floor(double tol, double rz_abs, double rz0) { return rz0 > 0.0 ? fmax(tol, sqrt(rz_abs / rz0)) : tol; }

// Forcing schedule: a LOOSE PCG iterate carries a component along the gauge direction eta_k = R_k v (all cameras rotated by the same v in their body
// frames: the exact null space of J^T J, held only by the LM damping, hence the last thing PCG resolves and invisible to its energy norm).  The
// exact step has none: v^T sum_k R_k^T Lam_k eta_k = 0 for every v, because the gradient is orthogonal to the gauge.  These two kernels remove it
// from an inexact step the same way -- w = (sum R^T Lam R)^-1 sum R^T Lam eta, eta_k -= R_k w -- and keep the PCG residual consistent
// (r += Lam R_k w; J^T J R w = 0), so that the model decrease computed from (eta, r) stays exact for the corrected step.
// Out of place (eta_out, rcg_out): the PCG state itself must stay what the stopping iteration left, so that the solve can be continued.
struct GaugeArgs { uint32_t n; int nb; const double* active; const double2* q; const double* Lam; const double* eta; const double* rcg; double* part; /* [9][nb] */ };
__global__ void __launch_bounds__(GSFM_BLOCK) k_gauge_part(GaugeArgs a) {
  __shared__ double lds[8];
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n && a.active[k] != 0.0) {
    double R[9], le[3];
    qmat(load_q(a.q, k), R);
    const double* L = a.Lam + 6 * (size_t)k;
    sym3_mulvec(L, a.eta + 3 * (size_t)k, le);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = R[c] * le[0] + R[3 + c] * le[1] + R[6 + c] * le[2];   // R^T Lam eta
    // R^T Lam R (symmetric: 00 01 02 11 12 22)
    double LR[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      LR[c] = L[0] * R[c] + L[1] * R[3 + c] + L[2] * R[6 + c];
      LR[3 + c] = L[1] * R[c] + L[3] * R[3 + c] + L[4] * R[6 + c];
      LR[6 + c] = L[2] * R[c] + L[4] * R[3 + c] + L[5] * R[6 + c];
    }
    v[3] = R[0] * LR[0] + R[3] * LR[3] + R[6] * LR[6]; v[4] = R[0] * LR[1] + R[3] * LR[4] + R[6] * LR[7]; v[5] = R[0] * LR[2] + R[3] * LR[5] + R[6] * LR[8];
    v[6] = R[1] * LR[1] + R[4] * LR[4] + R[7] * LR[7]; v[7] = R[1] * LR[2] + R[4] * LR[5] + R[7] * LR[8]; v[8] = R[2] * LR[2] + R[5] * LR[5] + R[8] * LR[8];
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const double t = block_sum_bcast(v[c], lds);
    if (threadIdx.x == 0) a.part[(size_t)c * a.nb + blockIdx.x] = t;
  }
}
// w = A^-1 s from the nine sums of k_gauge_part (every block: same partials, same order, same bits); a singular A (no damping at all) leaves
// the step alone.  All lanes of the workgroup must call it (block reductions).
__device__ __forceinline__ void gauge_solve(const double* __restrict__ part, int nb, double* lds, double* w) {
  double S[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) S[c] = sum_partials_bcast(part + (size_t)c * nb, nb, lds);
  const double a00 = S[3], a01 = S[4], a02 = S[5], a11 = S[6], a12 = S[7], a22 = S[8];
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const bool ok = fabs(det) > 0.0;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01, id = ok ? 1.0 / det : 0.0;
  w[0] = id * (c00 * S[0] + c01 * S[1] + c02 * S[2]); w[1] = id * (c01 * S[0] + c11 * S[1] + c12 * S[2]); w[2] = id * (c02 * S[0] + c12 * S[1] + c22 * S[2]);
}
// the correction of camera k: eta_k - R_k w and rcg_k + Lam_k R_k w (inactive cameras: unchanged)
__device__ __forceinline__ void gauge_correct(const double* w, bool active, const double2* __restrict__ q, const double* __restrict__ Lam, uint32_t k, const double* eta_in, const double* rcg_in, double* e, double* rc) {
  double d[3] = {0.0, 0.0, 0.0}, ld[3] = {0.0, 0.0, 0.0};
  if (active) {
    double R[9];
    qmat(load_q(q, k), R);
    d[0] = R[0] * w[0] + R[1] * w[1] + R[2] * w[2]; d[1] = R[3] * w[0] + R[4] * w[1] + R[5] * w[2]; d[2] = R[6] * w[0] + R[7] * w[1] + R[8] * w[2];
    sym3_mulvec(Lam + 6 * (size_t)k, d, ld);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { e[c] = eta_in[3 * (size_t)k + c] - d[c]; rc[c] = rcg_in[3 * (size_t)k + c] + ld[c]; }
}

struct StepArgs {
  uint32_t n;
  int param_dim;
  const double* x;        // current state
  const double* active;   // 1.0 for cameras touched by an edge
  const double* eta;      // PCG solution (left-tangent step)
  const double* b;        // -g_eta
  const double* rcg;      // PCG residual b - A eta
  const double* Lam;      // 6
  const double* Tinv;     // 9
  double* x_trial;
  double2* q_trial;
  double* partials;       // 6 * gridDim.x : eta.g, eta.rcg, eta^T Lam eta, |x - x_trial|^2, |x_trial|^2, sum_k |Tinv Minv rcg|_k^8 (0 unless Minv is given)
  const double* Minv;     // non-null (a loose PCG iterate, round 5): the sixth sum -- what block-Jacobi says each camera's step still lacks, in the
                          // units of the update (radians; half-angles for the quaternion state).  The energy norm the loose solve stops on weights a
                          // camera by its own weight sum: a camera whose edges are nearly all cut off by a redescending loss is invisible to it
                          // and can be left 1e-4 rad from its exact step under an energy error of 1e-8 (tests/manual/fuzz_forcing.py dense 5:14,
                          // 6:52: Tukey on ROTATION_MAT_FNORM).  The eighth-power sum is a smooth maximum: its 8th root lies between the largest
                          // camera's value and N^(1/8) times it (4.2 x at 100k cameras); lm_solve holds it against 10 x the rms tolerance.
  // a loose PCG iterate (forcing schedule): the nine sums of k_gauge_part; the gauge component is taken out of eta and the residual corrected
  // on the fly (round 4: the kernel that wrote the corrected copies is gone -- one launch fewer per loose step; the PCG state stays untouched)
  const double* gauge_part; int gauge_nb; const double2* gauge_q;
};
// delta = Tinv eta; x_trial = Plus(x, delta); scalars for the model cost change and the
// parameter-tolerance test (TrustRegionMinimizer::ComputeCandidatePointAndEvaluateCost).
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_step(StepArgs a) {
  __shared__ double lds[8];
  double v[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  double gw[3] = {0.0, 0.0, 0.0};
  if (a.gauge_part) gauge_solve(a.gauge_part, a.gauge_nb, lds, gw);
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    double e[3] = {a.eta[k3], a.eta[k3 + 1], a.eta[k3 + 2]}, rc[3] = {a.rcg[k3], a.rcg[k3 + 1], a.rcg[k3 + 2]};
    if (a.gauge_part) gauge_correct(gw, a.active[k] != 0.0, a.gauge_q, a.Lam, k, a.eta, a.rcg, e, rc);
    const double* Ti = a.Tinv + 9 * (size_t)k;
    const double d[3] = {Ti[0] * e[0] + Ti[1] * e[1] + Ti[2] * e[2], Ti[3] * e[0] + Ti[4] * e[1] + Ti[5] * e[2],
                         Ti[6] * e[0] + Ti[7] * e[1] + Ti[8] * e[2]};
    double le[3];
    sym3_mulvec(a.Lam + 6 * (size_t)k, e, le);
    v[0] = -(e[0] * a.b[k3] + e[1] * a.b[k3 + 1] + e[2] * a.b[k3 + 2]);
    v[1] = e[0] * rc[0] + e[1] * rc[1] + e[2] * rc[2];
    v[2] = e[0] * le[0] + e[1] * le[1] + e[2] * le[2];
    const double act = a.active[k];
    if (a.Minv) {
      double z[3];
      sym3_mulvec(a.Minv + 6 * (size_t)k, rc, z);
      const double dz0 = Ti[0] * z[0] + Ti[1] * z[1] + Ti[2] * z[2], dz1 = Ti[3] * z[0] + Ti[4] * z[1] + Ti[5] * z[2], dz2 = Ti[6] * z[0] + Ti[7] * z[1] + Ti[8] * z[2];
      const double m2 = act * (dz0 * dz0 + dz1 * dz1 + dz2 * dz2), m4 = m2 * m2;
      v[5] = m4 * m4;
    }
    Quat qt;
    if (a.param_dim == 3) {
      const double x0 = a.x[k3] + d[0], x1 = a.x[k3 + 1] + d[1], x2 = a.x[k3 + 2] + d[2];
      a.x_trial[k3] = x0; a.x_trial[k3 + 1] = x1; a.x_trial[k3 + 2] = x2;
      v[3] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      v[4] = act * (x0 * x0 + x1 * x1 + x2 * x2);
      qt = aa_to_quat(x0, x1, x2);
    } else {
      const size_t k4 = 4 * (size_t)k;
      const Quat q{a.x[k4], a.x[k4 + 1], a.x[k4 + 2], a.x[k4 + 3]};
      const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      qt = q;
      if (nd > 0.0) {
        double sn, cs;
        sincos(nd, &sn, &cs);
        const double kk = sn / nd;
        qt = qmul(Quat{kk * d[0], kk * d[1], kk * d[2], cs}, q);
      }
      a.x_trial[k4] = qt.x; a.x_trial[k4 + 1] = qt.y; a.x_trial[k4 + 2] = qt.z; a.x_trial[k4 + 3] = qt.w;
      const double f0 = q.x - qt.x, f1 = q.y - qt.y, f2 = q.z - qt.z, f3 = q.w - qt.w;
      v[3] = f0 * f0 + f1 * f1 + f2 * f2 + f3 * f3;
      v[4] = act * (qt.x * qt.x + qt.y * qt.y + qt.z * qt.z + qt.w * qt.w);
    }
    a.q_trial[2 * (size_t)k] = make_double2(qt.x, qt.y);
    a.q_trial[2 * (size_t)k + 1] = make_double2(qt.z, qt.w);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double t = block_sum_bcast(v[c], lds);
    if (threadIdx.x == 0) a.partials[(size_t)c * gridDim.x + blockIdx.x] = t;
  }
}
// out[c] = sum partials[c*n .. c*n+n)
__global__ void __launch_bounds__(GSFM_BLOCK) k_sum_partials_multi(const double* __restrict__ partials, int n, int m, double* out) {
  __shared__ double lds[8];
  for (int c = 0; c < m; ++c) {
    const double t = sum_partials_bcast(partials + (size_t)c * n, n, lds);
    if (threadIdx.x == 0) out[c] = t;
  }
}
// |x|^2 over active cameras (Init: x_norm_)
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_norm(const double* __restrict__ x, const double* __restrict__ active,
                                                         uint32_t n, int param_dim, double* partials) {
  __shared__ double lds[8];
  double v = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < n && active[k] != 0.0) {
    for (int c = 0; c < param_dim; ++c) { const double t = x[(size_t)param_dim * k + c]; v += t * t; }
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// export gradient / diagonal blocks in the reference's parameter space: T^T g, T^T D T
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_export(const double* __restrict__ x, const double* __restrict__ gD,
                                                           uint32_t n, int param_dim, double* grad, double* blocks, double* D6) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k >= n) return;
  double T[9], Ti[9];
  cam_tangent_maps(x, k, param_dim, T, Ti);
  const double* gd = gD + 9 * (size_t)k;
  const double D[9] = {gd[3], gd[4], gd[5], gd[4], gd[6], gd[7], gd[5], gd[7], gd[8]};
  double DT[9], TDT[9];
  mat3_mul(D, T, DT);
  mat3_tmul(T, DT, TDT);
  for (int c = 0; c < 3; ++c) grad[3 * (size_t)k + c] = T[c] * gd[0] + T[3 + c] * gd[1] + T[6 + c] * gd[2];
  for (int c = 0; c < 9; ++c) blocks[9 * (size_t)k + c] = TDT[c];
  for (int c = 0; c < 6; ++c) D6[6 * (size_t)k + c] = gd[3 + c];
}
// v_eta = T v (mode 0)  or  y = T^T y_eta (mode 1), for gsfm_rot_normal_matvec
__global__ void __launch_bounds__(GSFM_BLOCK) k_cam_apply_T(const double* __restrict__ x, uint32_t n, int param_dim, int transpose,
                                                            const double* __restrict__ in, double* __restrict__ out) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k >= n) return;
  double T[9], Ti[9];
  cam_tangent_maps(x, k, param_dim, T, Ti);
  const double v0 = in[3 * (size_t)k], v1 = in[3 * (size_t)k + 1], v2 = in[3 * (size_t)k + 2];
  for (int c = 0; c < 3; ++c)
    out[3 * (size_t)k + c] = transpose ? (T[c] * v0 + T[3 + c] * v1 + T[6 + c] * v2) : (T[3 * c] * v0 + T[3 * c + 1] * v1 + T[3 * c + 2] * v2);
}

}  // namespace gsfm
