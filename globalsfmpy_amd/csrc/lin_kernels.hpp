// K2: the linearisation on the row-major block-CSR layout -- LinArgs, lin_rows, lin_rows_fast and their entry points k_lin, k_lin3,
// k_lin_fast.  Launched by launch_lin in solver_launch.hpp; LinArgs and the fast-path helpers are shared with K2c (colsort_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"
#include "setup_kernels.hpp"

namespace gsfm {

#ifndef GSFM_K2_ATTR
// K2 is latency-bound (profiles/r01_e_pmc_sq_valu.txt): at the compiler's free choice of 184 VGPRs only two waves fit a
// SIMD; asking for at least three costs no spill (168 VGPRs) and 7.5 % less time on C5.  Four would spill 37 VGPRs (2x slower).
#define GSFM_K2_ATTR __attribute__((amdgpu_waves_per_eu(3)))
#endif

// ------------------------------------------------------------------------------------------
// K2: linearise.  G lanes cooperate on one camera row of the block-CSR J^T J.
// ------------------------------------------------------------------------------------------
struct LinArgs {
  uint32_t n_rows;           // owned rows
  uint32_t row_base;         // global camera index of row 0
  uint32_t G;                // lanes per row (power of two, <= 64)
  const uint32_t* row_ptr;   // [n_rows + 1]
  const uint32_t* col;       // neighbour camera | role << 31 (role 1: the row camera is `second`)
  const uint32_t* eid;
  const double2 *qr0, *qr1;
  const double2 *w0, *w1, *w2;
  const double* ws;
  const double2* q;
  const DevLoss* loss;
  const double* rho_ext;
  double2 *h0, *h1, *h2, *h3;  // H block planes (row-major 3x3: h0=(H00,H01) h1=(H02,H10) h2=(H11,H12) h3=(H20,H21))
  double* h4;                  // H22
  double* gD;                  // 9 per camera: g(3), D sym(6: d00 d01 d02 d11 d12 d22)
  int lap;                     // 1: Laplacian form, planes h0..h2 hold the symmetric edge weight B (see lin_rows)
  const double* go;            // non-null: the launch is predicated -- it does nothing unless *go != 0 (device-side LM control: the step was accepted)
  int fast_ok;                 // host decision: the alpha = 0 fast path may be taken (kind and parameter signs of the loss checked in prepare_loss)
  SigmaDev sigma;              // sigma consensus: compute the weight of every directed entry from its unit-weight residual, store it
  double* ws_rw;               //   into the weight plane (= ws, writable) and use it
};

// LAP = true ("Laplacian form", functors that depend on R_j R_i^T only: angle-axis and quaternion-cosine): for those
// J_i = -J_j Q with Q = R_j R_i^T exactly (also after the Corrector, which multiplies both blocks from the left), hence
//   H_jj = G, H_ji = -G Q, H_ij = -Q^T G, H_ii = Q^T G Q   with G = J_j^T J_j,
// i.e. every off-diagonal block is the row camera's own symmetric G_k = J_k^T J_k times a rotation:
//   H_km p_m = -G_k R_k (R_m^T p_m)   =>   y_k = M_k p_k - sum_{d in row k} G_d (R_k u[col_d]),   u_m = R_m^T p_m.
// (In the body frame B = R_k^T G_k R_k is the same matrix from either end of the edge: a graph Laplacian with one symmetric
// 3x3 weight per edge.)  K2 then stores 6 doubles per directed entry instead of 9 (planes h0..h2), needs no neighbour
// Jacobian, and K3 streams 52 B per entry instead of 76; the rotation by the row's R_k is nine FMAs K3 has room for.
template <int F, int WM, int LM, bool LAP>
__device__ __forceinline__ void lin_rows(const LinArgs& a) {
  if (a.go && *a.go == 0.0) return;
  const LossView<LM> lv = loss_view<LM>(a.loss);   // (before the first store: scalar loads, see loss_dev.hpp)
  constexpr int R = ResDim<F>::R;
  const uint32_t G = a.G;
  const uint32_t t = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const uint32_t row = t / G, lane = t % G;
  const bool live = row < a.n_rows;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const uint32_t k = a.row_base + row;
    const Quat qk = load_q(a.q, k);
    const uint32_t end = a.row_ptr[row + 1];
    for (uint32_t d = a.row_ptr[row] + lane; d < end; d += G) {
      const uint32_t cr = __builtin_nontemporal_load(a.col + d);
      const uint32_t m = cr & 0x7fffffffu;
      const bool row_is_second = (cr >> 31) != 0;
      double2 r0, r1;
      qrel_load_nt<WM>(a.qr0, a.qr1, d, r0, r1);
      const Quat qr = qrel_quat<WM>(r0, r1);
      EdgeW W = load_w<WM>(a.w0, a.w1, a.w2, a.ws, d);
      const bool sig = F == F_AA && WM == W_SCALAR && a.sigma.on;
      if (sig) W.l00 = 1.0;
      const Quat qm = load_q(a.q, m);
      double r[R], Ai[3 * R], Aj[3 * R];
      if (row_is_second) edge_linearize<F, WM>(qm, qk, qr, W, r, Ai, Aj);
      else edge_linearize<F, WM>(qk, qm, qr, W, r, Ai, Aj);
      if (sig) {   // r, Ai, Aj are unweighted here: the weight comes from |e|^2 and multiplies all three
        double su = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) su += r[c] * r[c];
        const double w = sigma_weight(a.sigma, su);
        __builtin_nontemporal_store(w, a.ws_rw + d);
#pragma unroll
        for (int c = 0; c < R; ++c) r[c] *= w;
#pragma unroll
        for (int c = 0; c < 3 * R; ++c) { Ai[c] *= w; Aj[c] *= w; }
      }
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < R; ++c) s += r[c] * r[c];
      Rho3 rho;
      if (a.rho_ext) { const size_t o = 3 * (size_t)a.eid[d]; rho.r0 = a.rho_ext[o]; rho.r1 = a.rho_ext[o + 1]; rho.r2 = a.rho_ext[o + 2]; }
      else rho = loss_eval<LM>(lv, s);
      robustify<R>(rho, s, r, Ai, Aj);
      const double* Ar = row_is_second ? Aj : Ai;  // Jacobian of the row camera
      const double* Ac = row_is_second ? Ai : Aj;  // Jacobian of the neighbour (dead code when LAP)
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        double g = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) g += Ar[3 * c + x] * r[c];
        acc[x] += g;
      }
      double d00 = 0, d01 = 0, d02 = 0, d11 = 0, d12 = 0, d22 = 0;
#pragma unroll
      for (int c = 0; c < R; ++c) {
        const double x0 = Ar[3 * c], x1 = Ar[3 * c + 1], x2 = Ar[3 * c + 2];
        d00 += x0 * x0; d01 += x0 * x1; d02 += x0 * x2; d11 += x1 * x1; d12 += x1 * x2; d22 += x2 * x2;
      }
      acc[3] += d00; acc[4] += d01; acc[5] += d02; acc[6] += d11; acc[7] += d12; acc[8] += d22;
      // streamed out once, read back by K3: non-temporal stores avoid the write-allocate fetch that PMC showed
      // (FETCH_SIZE of this kernel was 1.8x its algorithmic reads, profiles/r01_c_pmc_hbm_traffic.txt)
      if (LAP) {
        // G = J_k^T J_k of the row camera, as is: H_km p_m = -G_k R_k (R_m^T p_m), the rotation by R_k is applied by K3
        nt_store2(a.h0 + d, d00, d01);
        nt_store2(a.h1 + d, d02, d11);
        nt_store2(a.h2 + d, d12, d22);
      } else {
        double H[9];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
#pragma unroll
          for (int y = 0; y < 3; ++y) {
            double h = 0.0;
#pragma unroll
            for (int c = 0; c < R; ++c) h += Ar[3 * c + x] * Ac[3 * c + y];
            H[3 * x + y] = h;
          }
        }
        nt_store2(a.h0 + d, H[0], H[1]);
        nt_store2(a.h1 + d, H[2], H[3]);
        nt_store2(a.h2 + d, H[4], H[5]);
        nt_store2(a.h3 + d, H[6], H[7]);
        __builtin_nontemporal_store(H[8], a.h4 + d);
      }
    }
  }
  // segmented reduction over the G lanes of the row (rows are G-aligned inside the wavefront)
  for (uint32_t off = G >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] += __shfl_down(acc[c], off, G);
  }
  if (live && lane == 0) {
    double* o = a.gD + 9 * (size_t)(a.row_base + row);
#pragma unroll
    for (int c = 0; c < 9; ++c) o[c] = acc[c];
  }
}
// K2, fast path: Laplacian form + a loss whose rho'' is never positive (every LM_SIMPLE leaf, nu = 3 MAGSAC) + no host callback.
// Ceres' Corrector then takes its alpha = 0 branch for EVERY edge (corrector.cc: `if ((sq_norm == 0.0) || (rho[2] <= 0.0))`): residual and
// Jacobians are scaled by sqrt(rho') and nothing else.  So this path evaluates, per directed entry, only what the row needs:
//   * the row camera's Jacobian alone (the neighbour's is never formed; the general path computes both and discards one),
//   * rho' alone (loss_rho1: for MAGSAC one exp and one exact division instead of two exp, a table gather and nine divisions),
//   * g and G = J^T J from the unscaled Jacobian, multiplied by rho' at the end (no sqrt).
// About a third fewer VALU instructions per entry than the general path (round 2: 891, 22 of them IEEE divisions); C5: 914 -> 710 us.
// Same values as lin_rows up to the rounding of sqrt(rho')^2 vs rho'.
struct LinStreams { double2 r0, r1; EdgeW W; };
template <int WM>
__device__ __forceinline__ LinStreams lin_load_streams(const LinArgs& a, uint32_t d) {
  LinStreams S;
  qrel_load_nt<WM>(a.qr0, a.qr1, d, S.r0, S.r1);
  S.W = load_w<WM>(a.w0, a.w1, a.w2, a.ws, d);
  return S;
}
// one directed entry: residual r, row-camera Jacobian Ar (3x3 row-major); returns nothing else
template <int F, int WM>
__device__ __forceinline__ void edge_lin_row(const Quat& qk, const Quat& qm, const Quat& qr, EdgeW& W, bool row_is_second,
                                             const SigmaDev& sg, double* ws_slot, double* r, double* Ar) {
  const Quat qi = row_is_second ? qm : qk, qj = row_is_second ? qk : qm;
  if (F == F_AA) {
    const Quat qe = qmul(qmul(qj, qconj(qi)), qconj(qr));
    double e[3], s, th;
    quat_log<true>(qe, e, &s, &th);
    if (WM == W_SCALAR && sg.on) {   // sigma consensus: e is the unit-weight residual
      W.l00 = sigma_weight(sg, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      __builtin_nontemporal_store(W.l00, ws_slot);
    }
    apply_w_vec<WM>(W, e, r);
    const double c = jlinv_coeff(th, s, fabs(qe.w));
    double B[9], Mx[9];
    jlinv_matrix(e, c, B);                 // de/d eta_j = J_l^-1(e)
    if (row_is_second) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Mx[k] = B[k];
    } else {                               // de/d eta_i = -J_l^-1(e)^T R_ij
      double Rij[9], T[9];
      qmat(qr, Rij);
      mat3_tmul(B, Rij, T);
#pragma unroll
      for (int k = 0; k < 9; ++k) Mx[k] = -T[k];
    }
    apply_w_mat<WM>(W, Mx, Ar);
  } else {  // F_QCOS
    const Quat a = qmul(qr, qconj(qmul(qj, qconj(qi))));
    r[0] = 2.0 * a.x; r[1] = 2.0 * a.y; r[2] = 2.0 * a.z;
    if (row_is_second) {
      Ar[0] = -a.w; Ar[1] = a.z;  Ar[2] = -a.y;
      Ar[3] = -a.z; Ar[4] = -a.w; Ar[5] = a.x;
      Ar[6] = a.y;  Ar[7] = -a.x; Ar[8] = -a.w;
    } else {
      const double K[9] = {a.w, a.z, -a.y, -a.z, a.w, a.x, a.y, -a.x, a.w};
      double Rij[9];
      qmat(qr, Rij);
      mat3_mul(K, Rij, Ar);
    }
  }
}
// g (3) and G = J_k^T J_k (6: 00 01 02 11 12 22) of one directed entry, Corrector applied.  FAST: the rho'' <= 0 path above; otherwise the
// general one (both Jacobians, full Corrector, host-callback rho) restricted to the row camera's block -- the Laplacian form needs no more.
template <int F, int WM, int LM, bool FAST>
__device__ __forceinline__ void lin_entry_eval(const LinArgs& a, const LossView<LM>& lv, uint32_t d, uint32_t cr, const Quat& qk, const Quat& qm, LinStreams S, double* g3, double* G6) {
  const Quat qr = qrel_quat<WM>(S.r0, S.r1);
  const bool row_is_second = (cr >> 31) != 0;
  if (FAST) {
    double r[3], Ar[9];
    edge_lin_row<F, WM>(qk, qm, qr, S.W, row_is_second, a.sigma, a.ws_rw + d, r, Ar);
    const double rho1 = loss_rho1<LM>(lv, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
#pragma unroll
    for (int x = 0; x < 3; ++x) g3[x] = rho1 * (Ar[x] * r[0] + Ar[3 + x] * r[1] + Ar[6 + x] * r[2]);
    G6[0] = rho1 * (Ar[0] * Ar[0] + Ar[3] * Ar[3] + Ar[6] * Ar[6]); G6[1] = rho1 * (Ar[0] * Ar[1] + Ar[3] * Ar[4] + Ar[6] * Ar[7]);
    G6[2] = rho1 * (Ar[0] * Ar[2] + Ar[3] * Ar[5] + Ar[6] * Ar[8]); G6[3] = rho1 * (Ar[1] * Ar[1] + Ar[4] * Ar[4] + Ar[7] * Ar[7]);
    G6[4] = rho1 * (Ar[1] * Ar[2] + Ar[4] * Ar[5] + Ar[7] * Ar[8]); G6[5] = rho1 * (Ar[2] * Ar[2] + Ar[5] * Ar[5] + Ar[8] * Ar[8]);
  } else {
    constexpr int R = ResDim<F>::R;
    EdgeW W = S.W;
    const bool sig = F == F_AA && WM == W_SCALAR && a.sigma.on;
    if (sig) W.l00 = 1.0;
    double r[R], Ai[3 * R], Aj[3 * R];
    if (row_is_second) edge_linearize<F, WM>(qm, qk, qr, W, r, Ai, Aj);
    else edge_linearize<F, WM>(qk, qm, qr, W, r, Ai, Aj);
    if (sig) {
      double su = 0.0;
#pragma unroll
      for (int c = 0; c < R; ++c) su += r[c] * r[c];
      const double w = sigma_weight(a.sigma, su);
      __builtin_nontemporal_store(w, a.ws_rw + d);
#pragma unroll
      for (int c = 0; c < R; ++c) r[c] *= w;
#pragma unroll
      for (int c = 0; c < 3 * R; ++c) { Ai[c] *= w; Aj[c] *= w; }
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < R; ++c) s += r[c] * r[c];
    Rho3 rho;
    if (a.rho_ext) { const size_t o = 3 * (size_t)a.eid[d]; rho.r0 = a.rho_ext[o]; rho.r1 = a.rho_ext[o + 1]; rho.r2 = a.rho_ext[o + 2]; }
    else rho = loss_eval<LM>(lv, s);
    robustify<R>(rho, s, r, Ai, Aj);
    const double* Ar = row_is_second ? Aj : Ai;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      double g = 0.0;
#pragma unroll
      for (int c = 0; c < R; ++c) g += Ar[3 * c + x] * r[c];
      g3[x] = g;
    }
    double d00 = 0, d01 = 0, d02 = 0, d11 = 0, d12 = 0, d22 = 0;
#pragma unroll
    for (int c = 0; c < R; ++c) {
      const double x0 = Ar[3 * c], x1 = Ar[3 * c + 1], x2 = Ar[3 * c + 2];
      d00 += x0 * x0; d01 += x0 * x1; d02 += x0 * x2; d11 += x1 * x1; d12 += x1 * x2; d22 += x2 * x2;
    }
    G6[0] = d00; G6[1] = d01; G6[2] = d02; G6[3] = d11; G6[4] = d12; G6[5] = d22;
  }
}
// The same entry in the BODY frame (K2c's fast path, angle-axis family): with E = Exp(e) = R_j R_i^T R_ij^T one has J_l^-1(e)^T = J_l^-1(e) E and
// R_ij R_i = E^T R_j, so the first camera's Jacobian -J_l^-1(e)^T R_ij, taken to its body frame, is -J_l^-1(e) R_j -- the NEGATIVE of the
// second camera's body-frame Jacobian A = W J_l^-1(e) R_j.  One formula serves both roles (no R_ij matrix, no role-dependent branch), the block
// B = rho' A^T A comes out in the body frame K3c wants (no R_k^T G R_k afterwards), and the row sums are rotated ONCE per row by the finishing
// kernel: g_k = R_k sum(gb), D_k = R_k (sum B) R_k^T.  ~57 multiply-adds fewer per entry than lin_entry_eval<FAST> + the conjugation.
#ifndef GSFM_K2C_SC
#define GSFM_K2C_SC true   // K2c's transcendental coefficients in scalar registers (frees ~60 VGPRs; A/B: -DGSFM_K2C_SC=false)
#endif
template <int WM, int LM>
__device__ __forceinline__ double lin_entry_body_aa(const LinArgs& a, const LossView<LM>& lv, uint32_t d, uint32_t cr, const Quat& qk, const Quat& qm, LinStreams S, double* gb3, double* B6) {
  const Quat qr = qrel_quat<WM>(S.r0, S.r1);
  const bool row_is_second = (cr >> 31) != 0;
  const Quat qi = row_is_second ? qm : qk, qj = row_is_second ? qk : qm;
  const Quat qe = qmul(qmul(qj, qconj(qi)), qconj(qr));
  double e[3], s, th, r[3];
  quat_log<GSFM_K2C_SC>(qe, e, &s, &th);
  if (WM == W_SCALAR && a.sigma.on) {   // sigma consensus: e is the unit-weight residual
    S.W.l00 = sigma_weight(a.sigma, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    __builtin_nontemporal_store(S.W.l00, a.ws_rw + d);
  }
  apply_w_vec<WM>(S.W, e, r);
  double Jm[9], Rj[9], JR[9], A[9];
  jlinv_matrix(e, jlinv_coeff(th, s, fabs(qe.w)), Jm);
  qmat(qj, Rj);
  mat3_mul(Jm, Rj, JR);
  apply_w_mat<WM>(S.W, JR, A);
  const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const double rho1 = loss_rho1<LM, GSFM_K2C_SC>(lv, sq);
  const double sg = row_is_second ? rho1 : -rho1;
#pragma unroll
  for (int x = 0; x < 3; ++x) gb3[x] = sg * (A[x] * r[0] + A[3 + x] * r[1] + A[6 + x] * r[2]);
  B6[0] = rho1 * (A[0] * A[0] + A[3] * A[3] + A[6] * A[6]); B6[1] = rho1 * (A[0] * A[1] + A[3] * A[4] + A[6] * A[7]);
  B6[2] = rho1 * (A[0] * A[2] + A[3] * A[5] + A[6] * A[8]); B6[3] = rho1 * (A[1] * A[1] + A[4] * A[4] + A[7] * A[7]);
  B6[4] = rho1 * (A[1] * A[2] + A[4] * A[5] + A[7] * A[8]); B6[5] = rho1 * (A[2] * A[2] + A[5] * A[5] + A[8] * A[8]);
  return sq;   // |r|^2: the fused trial evaluation of K2c adds 1/2 rho(sq) of the edge's first-camera entry to the cost
}
template <int F, int WM, int LM>
__device__ __forceinline__ void lin_rows_fast(const LinArgs& a) {
  if (a.go && *a.go == 0.0) return;
  const LossView<LM> lv = loss_view<LM>(a.loss);   // (before the first store: scalar loads, see loss_dev.hpp)
  const uint32_t G = a.G;
  const uint32_t t = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const uint32_t row = t / G, lane = t % G;
  const bool live = row < a.n_rows;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const Quat qk = load_q(a.q, a.row_base + row);
    const uint32_t end = a.row_ptr[row + 1];
    // (a software-pipelined form of this loop -- next trip's column and streams requested before the current trip is evaluated, its
    // neighbour quaternion after the block stores -- was measured twice and dropped: round 3, 705-719 us against 710 at C5; round 4, with
    // the loss leaf in scalar registers and three waves per SIMD without spills, 404-455 us against 411-456 on the 100k / 10M ANGLE_AXIS
    // problem (profiles/r04b_roll_ab.txt): three to five waves per SIMD already hide the round trips of this loop)
    for (uint32_t d = a.row_ptr[row] + lane; d < end; d += G) {
      const uint32_t cr = __builtin_nontemporal_load(a.col + d);
      const LinStreams S = lin_load_streams<WM>(a, d);
      const Quat qm = load_q(a.q, cr & 0x7fffffffu);
      double g3[3], G6[6];
      lin_entry_eval<F, WM, LM, true>(a, lv, d, cr, qk, qm, S, g3, G6);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += g3[c];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[3 + c] += G6[c];
      nt_store2(a.h0 + d, G6[0], G6[1]);
      nt_store2(a.h1 + d, G6[2], G6[3]);
      nt_store2(a.h2 + d, G6[4], G6[5]);
    }
  }
  for (uint32_t off = G >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] += __shfl_down(acc[c], off, G);
  }
  if (live && lane == 0) {
    double* o = a.gD + 9 * (size_t)(a.row_base + row);
#pragma unroll
    for (int c = 0; c < 9; ++c) o[c] = acc[c];
  }
}
template <int F, int WM, int LM>
__global__ void __launch_bounds__(GSFM_BLOCK) GSFM_K2_ATTR k_lin_fast(LinArgs a) { lin_rows_fast<F, WM, LM>(a); }

// Two entry points over the same body: `k_lin3` asks for at least three waves per SIMD, which is free (no spill) for the
// instantiations that matter and would spill for the general loss program and the 9-residual functor; the launcher picks.
template <int F, int WM, int LM, bool LAP>
__global__ void __launch_bounds__(GSFM_BLOCK) k_lin(LinArgs a) { lin_rows<F, WM, LM, LAP>(a); }
template <int F, int WM, int LM, bool LAP>
__global__ void __launch_bounds__(GSFM_BLOCK) GSFM_K2_ATTR k_lin3(LinArgs a) { lin_rows<F, WM, LM, LAP>(a); }

}  // namespace gsfm
