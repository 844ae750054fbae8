// What every rotation kernel shares: the functor / weighting enums and the launch constants, the deterministic wave and block
// reductions, the per-edge evaluation (EdgeW, edge_residual, edge_linearize, robustify), the plane loads and the 3- / 4-component
// coding of the measured rotation (qrel_*).  Device functions only; included by every kernel family header of the rotation path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "loss_dev.hpp"
#include "so3_dev.hpp"

namespace gsfm {

enum { F_AA = 0, F_QCOS = 1, F_QNORM = 2, F_RFNORM = 3 };
enum { W_NONE = 0, W_SCALAR = 1, W_MATRIX = 2, W_MATRIX3 = 3 /* W_MATRIX with the measurement planes as three quaternion components (qrel_three below): a kernel template value only, never a problem's wmode */ };

template <int F> struct ResDim { static constexpr int R = (F == F_QNORM) ? 4 : (F == F_RFNORM) ? 9 : 3; };

#define GSFM_BLOCK 256
#define GSFM_MAX_PARTIALS 1024
// K1 tiles: cost edges are bucketed by (camera block of `first`, camera block of `second`), 2048 cameras per block;
// a 1024-thread workgroup stages BOTH quaternion blocks in LDS (2 x 2048 x 32 B = 128 KiB of the 160 KiB), so the
// sweep performs no global gather at all.
#define GSFM_CAMBLOCK 2048

// ------------------------------------------------------------------------------------------
// reductions (deterministic: fixed tree inside a wave, fixed order across waves)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}
// result valid in every thread
__device__ __forceinline__ double block_sum_bcast(double v, double* lds /* >= 5 */) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0; for (int k = 0; k < GSFM_BLOCK / 64; ++k) t += lds[k]; lds[4] = t; }
  __syncthreads();
  return lds[4];
}
__device__ __forceinline__ double block_max_bcast(double v, double* lds) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double t = lds[0]; for (int k = 1; k < GSFM_BLOCK / 64; ++k) t = fmax(t, lds[k]); lds[4] = t; }
  __syncthreads();
  return lds[4];
}
// every block sums the same `n` partials in the same order -> identical scalar in every block
__device__ __forceinline__ double sum_partials_bcast(const double* __restrict__ partials, int n, double* lds) {
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += GSFM_BLOCK) v += partials[k];
  return block_sum_bcast(v, lds);
}

// ------------------------------------------------------------------------------------------
// per-edge evaluation
// ------------------------------------------------------------------------------------------
struct EdgeW { double l00, l01, l02, l11, l12, l22; };  // upper-triangular whitening factor / scalar in l00

template <int WM>
__device__ __forceinline__ void apply_w_vec(const EdgeW& W, const double* e, double* r) {
  if (WM == W_NONE) { r[0] = e[0]; r[1] = e[1]; r[2] = e[2]; }
  else if (WM == W_SCALAR) { r[0] = W.l00 * e[0]; r[1] = W.l00 * e[1]; r[2] = W.l00 * e[2]; }
  else {
    r[0] = W.l00 * e[0] + W.l01 * e[1] + W.l02 * e[2];
    r[1] = W.l11 * e[1] + W.l12 * e[2];
    r[2] = W.l22 * e[2];
  }
}
template <int WM>
__device__ __forceinline__ void apply_w_mat(const EdgeW& W, const double* M, double* O) {  // O = W M
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (WM == W_NONE) { O[c] = M[c]; O[3 + c] = M[3 + c]; O[6 + c] = M[6 + c]; }
    else if (WM == W_SCALAR) { O[c] = W.l00 * M[c]; O[3 + c] = W.l00 * M[3 + c]; O[6 + c] = W.l00 * M[6 + c]; }
    else {
      O[c] = W.l00 * M[c] + W.l01 * M[3 + c] + W.l02 * M[6 + c];
      O[3 + c] = W.l11 * M[3 + c] + W.l12 * M[6 + c];
      O[6 + c] = W.l22 * M[6 + c];
    }
  }
}

// Residual only.  qi, qj: camera quaternions of (first, second); qr: measured R_ij.
template <int F, int WM>
__device__ __forceinline__ void edge_residual(const Quat& qi, const Quat& qj, const Quat& qr, const EdgeW& W, double* r) {
  if (F == F_AA) {
    // e = log(R_j R_i^T R_ij^T)   (Theia pairwise_rotation_error.h:80-92 / quat.hpp:231-246)
    const Quat qe = qmul(qmul(qj, qconj(qi)), qconj(qr));
    double e[3], s, th;
    quat_log(qe, e, &s, &th);
    apply_w_vec<WM>(W, e, r);
  } else if (F == F_QCOS) {
    // r = 2 vec(q_ij * (q_b * q_a^-1)^*)   (quat.hpp:86-103)
    const Quat dq = qmul(qr, qconj(qmul(qj, qconj(qi))));
    r[0] = 2.0 * dq.x; r[1] = 2.0 * dq.y; r[2] = 2.0 * dq.z;
  } else if (F == F_QNORM) {
    // r = canon(q_b) - canon(q_ij q_a), canon tests the y coefficient  (quat.hpp:130-147)
    const Quat est = qmul(qr, qi);
    const double sb = (qj.y < 0.0) ? -1.0 : 1.0, se = (est.y < 0.0) ? -1.0 : 1.0;
    r[0] = sb * qj.x - se * est.x; r[1] = sb * qj.y - se * est.y;
    r[2] = sb * qj.z - se * est.z; r[3] = sb * qj.w - se * est.w;
  } else {
    // r = vec_colmajor(R_ij R_a - R_b)   (quat.hpp:170-193)
    double Est[9], Rb[9];
    qmat(qmul(qr, qi), Est);
    qmat(qj, Rb);
#pragma unroll
    for (int k = 0; k < 9; ++k) { const int rr = k % 3, cc = k / 3; r[k] = Est[3 * rr + cc] - Rb[3 * rr + cc]; }
  }
}

__device__ __forceinline__ void plus_jac_half(const Quat& q, double sgn, double* P /*4x3*/) {
  // 1/2 * d((h,1) (x) q)/dh : rows x,y,z,w  (ceres EigenQuaternionParameterization::ComputeJacobian, eta = 2 delta)
  const double h = 0.5 * sgn;
  P[0] = h * q.w;  P[1] = h * q.z;   P[2] = -h * q.y;
  P[3] = -h * q.z; P[4] = h * q.w;   P[5] = h * q.x;
  P[6] = h * q.y;  P[7] = -h * q.x;  P[8] = h * q.w;
  P[9] = -h * q.x; P[10] = -h * q.y; P[11] = -h * q.z;
}

// Residual and body Jacobians A_i, A_j (R x 3, row-major) w.r.t. left perturbations of R_i, R_j.
template <int F, int WM>
__device__ __forceinline__ void edge_linearize(const Quat& qi, const Quat& qj, const Quat& qr, const EdgeW& W,
                                               double* r, double* Ai, double* Aj) {
  if (F == F_AA) {
    const Quat qe = qmul(qmul(qj, qconj(qi)), qconj(qr));
    double e[3], s, th;
    quat_log(qe, e, &s, &th);
    apply_w_vec<WM>(W, e, r);
    const double c = jlinv_coeff(th, s, fabs(qe.w));
    double B[9], Rij[9], Bt_R[9];
    jlinv_matrix(e, c, B);            // de/d eta_j = J_l^-1(e)
    apply_w_mat<WM>(W, B, Aj);
    qmat(qr, Rij);
    mat3_tmul(B, Rij, Bt_R);          // de/d eta_i = -J_r^-1(e) R_ij = -J_l^-1(e)^T R_ij
#pragma unroll
    for (int k = 0; k < 9; ++k) Bt_R[k] = -Bt_R[k];
    apply_w_mat<WM>(W, Bt_R, Ai);
  } else if (F == F_QCOS) {
    const Quat a = qmul(qr, qconj(qmul(qj, qconj(qi))));
    r[0] = 2.0 * a.x; r[1] = 2.0 * a.y; r[2] = 2.0 * a.z;
    Aj[0] = -a.w; Aj[1] = a.z;  Aj[2] = -a.y;
    Aj[3] = -a.z; Aj[4] = -a.w; Aj[5] = a.x;
    Aj[6] = a.y;  Aj[7] = -a.x; Aj[8] = -a.w;
    const double K[9] = {a.w, a.z, -a.y, -a.z, a.w, a.x, a.y, -a.x, a.w};
    double Rij[9];
    qmat(qr, Rij);
    mat3_mul(K, Rij, Ai);
  } else if (F == F_QNORM) {
    const Quat est = qmul(qr, qi);
    const double sb = (qj.y < 0.0) ? -1.0 : 1.0, se = (est.y < 0.0) ? -1.0 : 1.0;
    r[0] = sb * qj.x - se * est.x; r[1] = sb * qj.y - se * est.y;
    r[2] = sb * qj.z - se * est.z; r[3] = sb * qj.w - se * est.w;
    plus_jac_half(qj, sb, Aj);
    double P[12], Rij[9];
    plus_jac_half(est, -se, P);
    qmat(qr, Rij);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) Ai[3 * k + c] = P[3 * k] * Rij[c] + P[3 * k + 1] * Rij[3 + c] + P[3 * k + 2] * Rij[6 + c];
  } else {
    double Est[9], Rb[9], Rij[9];
    qmat(qmul(qr, qi), Est);
    qmat(qj, Rb);
    qmat(qr, Rij);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const double u0 = Rb[cc], u1 = Rb[3 + cc], u2 = Rb[6 + cc];        // column cc of R_b
      const double v0 = Est[cc], v1 = Est[3 + cc], v2 = Est[6 + cc];     // column cc of R_ij R_a
      r[3 * cc] = v0 - u0; r[3 * cc + 1] = v1 - u1; r[3 * cc + 2] = v2 - u2;
      // d(-R_b col)/d eta_j = [u]x
      double* J = Aj + 9 * cc;
      J[0] = 0.0; J[1] = -u2; J[2] = u1;
      J[3] = u2;  J[4] = 0.0; J[5] = -u0;
      J[6] = -u1; J[7] = u0;  J[8] = 0.0;
      // d(Est col)/d eta_i = -[v]x R_ij
      const double K[9] = {0.0, v2, -v1, -v2, 0.0, v0, v1, -v0, 0.0};
      mat3_mul(K, Rij, Ai + 9 * cc);
    }
  }
}

// Ceres ResidualBlock::Evaluate + Corrector applied in place; returns 1/2 rho.
template <int R>
__device__ __forceinline__ void robustify(const Rho3& rho, double s, double* r, double* Ai, double* Aj) {
  const Corrector c = make_corrector(s, rho);
  if (c.alpha_sq_norm == 0.0) {
#pragma unroll
    for (int k = 0; k < 3 * R; ++k) { Ai[k] *= c.sqrt_rho1; Aj[k] *= c.sqrt_rho1; }
  } else {
#pragma unroll
    for (int col = 0; col < 3; ++col) {
      double ti = 0.0, tj = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) { ti += Ai[3 * k + col] * r[k]; tj += Aj[3 * k + col] * r[k]; }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        Ai[3 * k + col] = c.sqrt_rho1 * (Ai[3 * k + col] - c.alpha_sq_norm * r[k] * ti);
        Aj[3 * k + col] = c.sqrt_rho1 * (Aj[3 * k + col] - c.alpha_sq_norm * r[k] * tj);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) r[k] *= c.residual_scaling;
}

__device__ __forceinline__ double2 nt_load2(const double2* __restrict__ p) {
  double2 v;
  v.x = __builtin_nontemporal_load(&p->x);
  v.y = __builtin_nontemporal_load(&p->y);
  return v;
}
__device__ __forceinline__ void nt_store2(double2* __restrict__ p, double x, double y) {
  __builtin_nontemporal_store(x, &p->x);
  __builtin_nontemporal_store(y, &p->y);
}
template <int WM>
__device__ __forceinline__ EdgeW load_w(const double2* __restrict__ w0, const double2* __restrict__ w1,
                                        const double2* __restrict__ w2, const double* __restrict__ ws, size_t e) {
  EdgeW W;
  W.l00 = 1.0; W.l01 = W.l02 = W.l12 = 0.0; W.l11 = W.l22 = 1.0;
  if (WM == W_SCALAR) { W.l00 = __builtin_nontemporal_load(ws + e); }
  else if (WM == W_MATRIX || WM == W_MATRIX3) {
    const double2 a = nt_load2(w0 + e), b = nt_load2(w1 + e), c = nt_load2(w2 + e);
    W.l00 = a.x; W.l01 = a.y; W.l02 = b.x; W.l11 = b.y; W.l12 = c.x; W.l22 = c.y;
  }
  return W;
}
__device__ __forceinline__ Quat load_q(const double2* __restrict__ q2, uint32_t k) {
  const double2 a = q2[2 * (size_t)k], b = q2[2 * (size_t)k + 1];
  return Quat{a.x, a.y, b.x, b.y};
}

// ------------------------------------------------------------------------------------------
// The measured relative rotation of an edge / a directed entry: 24 bytes per position on covariance-whitened problems (round 6; SURVEY 8(d)
// counts the measurement at 24 B).  A unit quaternion is three numbers and a sign: the component of LARGEST magnitude (>= 1/2) is dropped and
// rebuilt as +-sqrt(1 - a^2 - b^2 - c^2); dropping the largest keeps the rebuilt one accurate to an ulp (dropping w outright would lose
// ~1e-16 / w: a third of the benchmark's edges are uniformly random rotations, |w| < 1e-4 on hundreds of them).  Which component was dropped
// (0..3 = x, y, z, w) rides in bit 62 of the first two stored doubles -- the top bit of the exponent field, zero for every |value| < 2 -- and
// its sign in bit 62 of the third (q and -q are the same rotation, but the quaternion-cosine residual, quat.hpp:86-103, carries the sign of
// q_ij into the sign of r: the stored quaternion is the one ceres::AngleAxisToQuaternion gives, not a normalised one).
// Planes: qr0 = (a, b) as double2, qr1 = c as double (the buffer is still handed around as a double2 pointer).
// WHERE: the W_MATRIX problems (ANGLE_AXIS_COVARIANCE / COV_INLIERS: 88 -> 80 B streamed per edge) of at least one million edges -- where the
// sweeps are bound by the stream (gsfm_rot_problem::q3, decided at create: such a problem launches the W_MATRIX3 instantiations; GSFM_QREL3=0/1 in the
// environment overrides).  Below that size the
// launches are bound by latency, the 8 bytes buy nothing, and the rebuilt component -- within an ulp of ceres::AngleAxisToQuaternion's, not always
// equal to it -- would move the small configurations' last bits for no gain: on the real Madrid graph under MAGSAC, whose outcome is bimodal under
// one-ulp changes of the measurements, it was enough to land the run in the other cluster (62 instead of 63 LM iterations, 2.0e-4
// rad from the unperturbed oracle: profiles/r06_bench_madrid_with_q3.json).  Measured at C5, same box, alternating
// (profiles/r06_qrel3_ab.txt): reweight sweep 180 -> 168.5 us (0.61 -> 0.65 of the roofline on SURVEY 8(d)'s bytes), full sweep 221 -> 213.5, s-only
// 172 -> 166.5, K2c 580-593 -> 583-587 (its own stream is not what binds it), the trial-cost sweep 137.4 -> 142.2 (it stores nothing and is bound
// by instruction issue: the ~45 VALU operations of the decode show), a whole solve 12.01 -> 11.94 ms with the final cost equal to the last bit.  The
// unit- and scalar-weight sweeps (40-48 B per edge) are bound by instruction issue throughout -- 98.6 -> 108.4 us with three components -- and
// keep the full quaternion, 32 B.  -DGSFM_QREL3=0: the full quaternion everywhere (rounds 1-5).
#ifndef GSFM_QREL3
#define GSFM_QREL3 1
#endif
// (A compile-time property of the kernels -- the template value W_MATRIX3 -- not a runtime branch inside the W_MATRIX ones: with the branch compiled
// in, the compiler scheduled the W_MATRIX kernels' arithmetic differently, last bits of the small configurations moved, and Madrid / MAGSAC -- bimodal
// under one-ulp changes, DESIGN section 2 -- landed in its other cluster, 62 instead of 63 LM iterations: profiles/r06_madrid_bits.txt.)
__host__ __device__ constexpr bool qrel_three(int wm) { return GSFM_QREL3 != 0 && wm == W_MATRIX3; }
__device__ __forceinline__ void qrel_encode(const Quat& q, double* ab_c /* [3] */) {
  const double v[4] = {q.x, q.y, q.z, q.w};
  if (!(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]))) { ab_c[0] = ab_c[1] = ab_c[2] = 1.5; return; }   // a non-finite measurement decodes to NaN (1 - 3 x 2.25 < 0)
  int k = 3;
  double m = fabs(v[3]);
#pragma unroll
  for (int c = 2; c >= 0; --c) if (fabs(v[c]) > m) { m = fabs(v[c]); k = c; }
  double o[3];
  int n = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) if (c != k) o[n++] = v[c];
  unsigned long long b0 = (unsigned long long)__double_as_longlong(o[0]), b1 = (unsigned long long)__double_as_longlong(o[1]), b2 = (unsigned long long)__double_as_longlong(o[2]);
  b0 |= (unsigned long long)(k & 1) << 62; b1 |= (unsigned long long)(k >> 1) << 62; b2 |= (unsigned long long)(v[k] < 0.0 ? 1 : 0) << 62;
  ab_c[0] = __longlong_as_double((long long)b0); ab_c[1] = __longlong_as_double((long long)b1); ab_c[2] = __longlong_as_double((long long)b2);
}
// raw: the full quaternion (x, y) (z, w) -- or, three components: (a, b) in r0, c in r1.x (r1.y unused)
template <int WM>
__device__ __forceinline__ Quat qrel_quat(const double2& r0, const double2& r1) {
  if constexpr (!qrel_three(WM)) return Quat{r0.x, r0.y, r1.x, r1.y};
  else {
    const unsigned ha = (unsigned)__double2hiint(r0.x), hb = (unsigned)__double2hiint(r0.y), hc = (unsigned)__double2hiint(r1.x);
    const unsigned k = ((ha >> 30) & 1u) | (((hb >> 30) & 1u) << 1);
    const double a = __hiloint2double((int)(ha & 0xbfffffffu), __double2loint(r0.x)), b = __hiloint2double((int)(hb & 0xbfffffffu), __double2loint(r0.y)),
                 c = __hiloint2double((int)(hc & 0xbfffffffu), __double2loint(r1.x));
    const double mp = sqrt(1.0 - a * a - b * b - c * c);   // (>= 1/4 for a unit quaternion; negative -> NaN for what qrel_encode made of a non-finite one)
    const double m = __hiloint2double(__double2hiint(mp) ^ (int)((hc << 1) & 0x80000000u), __double2loint(mp));   // (bit 30 of the third's high word -> the sign bit)
    Quat q;   // stored order = (x, y, z, w) with component k removed
    q.x = k == 0u ? m : a;
    q.y = k == 0u ? a : (k == 1u ? m : b);
    q.z = k == 3u ? c : (k == 2u ? m : b);
    q.w = k == 3u ? m : c;
    return q;
  }
}
template <int WM>
__device__ __forceinline__ void qrel_load_nt(const double2* __restrict__ qr0, const double2* __restrict__ qr1, size_t e, double2& r0, double2& r1) {
  r0 = nt_load2(qr0 + e);
  if constexpr (qrel_three(WM)) { r1.x = __builtin_nontemporal_load((const double*)qr1 + e); r1.y = 0.0; } else r1 = nt_load2(qr1 + e);
}
template <int WM>
__device__ __forceinline__ void qrel_load(const double2* __restrict__ qr0, const double2* __restrict__ qr1, size_t e, double2& r0, double2& r1) {
  r0 = qr0[e];
  if constexpr (qrel_three(WM)) { r1.x = ((const double*)qr1)[e]; r1.y = 0.0; } else r1 = qr1[e];
}

}  // namespace gsfm
