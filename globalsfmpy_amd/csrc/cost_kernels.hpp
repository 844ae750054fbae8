// K1: the cost sweep over the cost-owned edges -- k_cost (LDS-tiled), k_cost_direct, k_loss_eval, k_sum_partials.  Arguments are built
// by cost_args and launched by launch_cost in solver_launch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"
#include "setup_kernels.hpp"

namespace gsfm {

#ifndef GSFM_TILE_THREADS
#define GSFM_TILE_THREADS 1024
#endif
#ifndef GSFM_K1_UNROLL
#define GSFM_K1_UNROLL 1   // edges per lane whose streams are requested before any of them is evaluated
#endif

// ------------------------------------------------------------------------------------------
// K1: residual + robust reweight sweep over the cost-owned edges
// ------------------------------------------------------------------------------------------
struct CostTile { uint32_t ib, jb, begin, end; };  // camera blocks of (first, second), edge range
struct CostArgs {
  const CostTile* tiles;     // one per workgroup
  uint32_t n_cams;
  size_t n;                  // edges, ordered by tile; idx holds BLOCK-LOCAL camera indices
  const uint2* idx;          // (i, j)
  const double2 *qr0, *qr1;  // q_rel planes (x,y) (z,w) -- or (a,b), c in the W_MATRIX3 kernels
  const double2 *w0, *w1, *w2;
  const double* ws;
  const double2* q;          // camera quaternions
  const DevLoss* loss;
  const double* rho_ext;     // external rho triples per ORIGINAL edge (callback path) or null
  const uint32_t* eid;       // entry -> original edge (rho_ext only)
  double* partials;          // [gridDim.x] sum of 1/2 rho; FULL kernels: [2 * gridDim.x], second half = sum |w - w_old| (sigma mode)
  // optional per-edge outputs (null in the solver loop), in the PROBLEM's edge order (= the order of the streamed planes; position u holds
  // original edge gsfm_rot_edge_order()[u]): every store is a coalesced non-temporal 8 / 16 B per lane.  (Round 2 stored through `eid`
  // into the caller's order: 438 MB written for 320 MB of payload, 0.43 of the HBM roofline.)
  double* s_out;             // s alone (s_only mode)
  double2* srho_out;         // (s, rho)           } the full sweep: two 16-byte stores per lane
  double2* rho12_out;        // (rho', rho'')      }
  double* rho1_out;          // rho' alone: the reweight sweep of SURVEY 8(d) (8 B out per edge)
  double* r_out;             // residuals, R planes of n
  int s_only;                // 1: write s_out only, skip the loss (callback path, phase 1)
  int direct;                // 1: k_cost_direct (idx = global camera indices, tiles = plain chunks)
  int unit_w;                // 1: ignore the scalar weight plane
  SigmaDev sigma;            // sigma consensus: compute, store (ws_rw) and use the weights
  double* ws_rw;             // = ws, writable
};

// K1.  FULL = false: the solver's trial-cost sweep (cost only: for MAGSAC the value needs no exp and no division
// by constants).  FULL = true: per-edge outputs / external rho / s-only / sigma modes.  One edge per lane; the seven streamed planes
// are 16-byte coalesced, non-temporal loads; both camera quaternions come from LDS.  Measured (tools/bench_cost*.hip, C5): streams only
// 137 us; + all arithmetic 138-152 us (hidden); direct global gathers 181 us; these 2-D LDS tiles 160 us.
// One edge of K1: residual, s, loss, optional per-edge outputs; returns the edge's 1/2 rho (0 in s_only mode).
template <int F, int WM, int LM, int MODE>
__device__ __forceinline__ double cost_edge(const CostArgs& a, const LossView<LM>& lv, uint32_t e, const Quat& qi, const Quat& qj, const Quat& qr, EdgeW W, double& dw_acc) {
  constexpr int R = ResDim<F>::R;
  constexpr bool FULL = MODE == 1;   // MODE 0: cost only (trial sweeps); 1: every optional output, sigma consensus, host-callback rho; 2: the reweight sweep (rho' stored)
  double r[R];
  if (FULL && F == F_AA && WM == W_SCALAR && a.sigma.on) {
    const double w_old = W.l00;
    W.l00 = 1.0;
    edge_residual<F, WM>(qi, qj, qr, W, r);
    const double w = sigma_weight(a.sigma, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    dw_acc += fabs(w - w_old);
    __builtin_nontemporal_store(w, a.ws_rw + e);
#pragma unroll
    for (int k = 0; k < R; ++k) r[k] *= w;
  } else {
    edge_residual<F, WM>(qi, qj, qr, W, r);
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) s += r[k] * r[k];
  if (MODE == 0) return 0.5 * loss_value<LM>(lv, s);
  if (MODE == 2) {   // SURVEY 8(d)'s reweight sweep and nothing else: residual, loss, rho' out (8 B, coalesced, non-temporal), no run-time option in the way
    const Rho3 rho = loss_eval<LM>(lv, s);
    __builtin_nontemporal_store(rho.r1, a.rho1_out + e);
    return 0.5 * rho.r0;
  }
  if (a.s_only) { __builtin_nontemporal_store(s, a.s_out + e); return 0.0; }
  Rho3 rho;
  if (a.rho_ext) { const size_t o = 3 * (size_t)a.eid[e]; rho.r0 = a.rho_ext[o]; rho.r1 = a.rho_ext[o + 1]; rho.r2 = a.rho_ext[o + 2]; }
  else rho = loss_eval<LM>(lv, s);
  if (a.srho_out) nt_store2(a.srho_out + e, s, rho.r0);
  if (a.rho12_out) nt_store2(a.rho12_out + e, rho.r1, rho.r2);
  if (a.rho1_out) __builtin_nontemporal_store(rho.r1, a.rho1_out + e);
  if (a.r_out) {
#pragma unroll
    for (int k = 0; k < R; ++k) __builtin_nontemporal_store(r[k], a.r_out + (size_t)k * a.n + e);
  }
  return 0.5 * rho.r0;
}

template <int F, int WM, int LM, int MODE>
__global__ void __launch_bounds__(GSFM_TILE_THREADS) k_cost(CostArgs a) {
  __shared__ double2 qi_xy[GSFM_CAMBLOCK], qi_zw[GSFM_CAMBLOCK], qj_xy[GSFM_CAMBLOCK], qj_zw[GSFM_CAMBLOCK];
  __shared__ double lds[GSFM_TILE_THREADS / 64 + 1];
  const CostTile tile = a.tiles[blockIdx.x];
  const LossView<LM> lv = loss_view<LM>(a.loss);   // (before the first store: scalar loads, see loss_dev.hpp)
  {
    const uint32_t bi = tile.ib * GSFM_CAMBLOCK, bj = tile.jb * GSFM_CAMBLOCK;
    const uint32_t ci = min((uint32_t)GSFM_CAMBLOCK, a.n_cams - bi), cj = min((uint32_t)GSFM_CAMBLOCK, a.n_cams - bj);
    for (uint32_t c = threadIdx.x; c < ci; c += GSFM_TILE_THREADS) { qi_xy[c] = a.q[2 * (size_t)(bi + c)]; qi_zw[c] = a.q[2 * (size_t)(bi + c) + 1]; }
    for (uint32_t c = threadIdx.x; c < cj; c += GSFM_TILE_THREADS) { qj_xy[c] = a.q[2 * (size_t)(bj + c)]; qj_zw[c] = a.q[2 * (size_t)(bj + c) + 1]; }
  }
  __syncthreads();
  double acc = 0.0, dw = 0.0;
  constexpr int U = GSFM_K1_UNROLL;
  for (uint32_t e0 = tile.begin + threadIdx.x; e0 < tile.end; e0 += U * GSFM_TILE_THREADS) {
    // request phase: the streams of U edges are in flight before the first residual is evaluated
    uint2 ij[U];
    double2 r0[U], r1[U];
    EdgeW Wm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t eu = e0 + u * GSFM_TILE_THREADS;
      const uint32_t e = eu < tile.end ? eu : e0;   // lanes past the end re-read their first edge and discard it
      ij[u] = a.idx[e];
      qrel_load_nt<WM>(a.qr0, a.qr1, e, r0[u], r1[u]);
      Wm[u] = load_w<WM>(a.w0, a.w1, a.w2, a.ws, e);
      if (WM == W_SCALAR && a.unit_w) Wm[u].l00 = 1.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t e = e0 + u * GSFM_TILE_THREADS;
      if (e >= tile.end) continue;
      const Quat qr = qrel_quat<WM>(r0[u], r1[u]);
      const double2 i0 = qi_xy[ij[u].x], i1 = qi_zw[ij[u].x], j0 = qj_xy[ij[u].y], j1 = qj_zw[ij[u].y];
      const Quat qi{i0.x, i0.y, i1.x, i1.y}, qj{j0.x, j0.y, j1.x, j1.y};
      acc += cost_edge<F, WM, LM, MODE>(a, lv, e, qi, qj, qr, Wm[u], dw);
    }
  }
  // deterministic block reduction (fixed tree per wave, fixed order over the 16 waves)
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < GSFM_TILE_THREADS / 64; ++k) t += lds[k];
    a.partials[blockIdx.x] = t;
  }
  if (MODE == 1) {   // sum |w - w_old| of the sigma mode (zero otherwise)
    dw = wave_sum(dw);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = dw;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < GSFM_TILE_THREADS / 64; ++k) t += lds[k];
      a.partials[gridDim.x + blockIdx.x] = t;
    }
  }
}

// K1 without LDS staging, for sweeps whose (first block, second block) tiles are too thinly populated to amortise the
// 128 KiB fill -- many cameras at a fixed degree (edges per tile = degree * 2048^2 / cameras), or one rank's share of a
// sharded problem.  Same edge order (so a chunk's gathers fall into few 64 KiB windows of q), `idx` holds GLOBAL camera
// indices, the quaternions are gathered through L1/L2; 256 lanes per workgroup, no LDS, so the occupancy is VGPR-bound.
template <int F, int WM, int LM, int MODE>
__global__ void __launch_bounds__(GSFM_BLOCK) k_cost_direct(CostArgs a) {
  __shared__ double lds[GSFM_BLOCK / 64 + 1];
  const CostTile tile = a.tiles[blockIdx.x];
  const LossView<LM> lv = loss_view<LM>(a.loss);
  double acc = 0.0, dw = 0.0;
  for (uint32_t e = tile.begin + threadIdx.x; e < tile.end; e += GSFM_BLOCK) {
    const uint2 ij = a.idx[e];
    double2 r0, r1;
    qrel_load_nt<WM>(a.qr0, a.qr1, e, r0, r1);
    EdgeW W = load_w<WM>(a.w0, a.w1, a.w2, a.ws, e);
    if (WM == W_SCALAR && a.unit_w) W.l00 = 1.0;
    const Quat qi = load_q(a.q, ij.x), qj = load_q(a.q, ij.y);
    acc += cost_edge<F, WM, LM, MODE>(a, lv, e, qi, qj, qrel_quat<WM>(r0, r1), W, dw);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < GSFM_BLOCK / 64; ++k) t += lds[k];
    a.partials[blockIdx.x] = t;
  }
  if (MODE == 1) {
    dw = wave_sum(dw);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = dw;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < GSFM_BLOCK / 64; ++k) t += lds[k];
      a.partials[gridDim.x + blockIdx.x] = t;
    }
  }
}

// The loss program on given squared norms, through the very routines the sweeps use (device-level pin against the reference's
// recorded (s, rho, rho', rho'') vectors): rho3 = loss_eval<LM> (K2's general path and the FULL sweep), val = loss_value<LM> (the
// cost-only sweep), rho1 = loss_rho1<LM> (K2's fast path; LM_SIMPLE / LM_MAGSAC only).
template <int LM>
__global__ void __launch_bounds__(GSFM_BLOCK) k_loss_eval(const DevLoss* __restrict__ loss, const double* __restrict__ s, size_t n,
                                                          double* __restrict__ rho3, double* __restrict__ val, double* __restrict__ rho1) {
  const size_t t = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (t >= n) return;
  const double sq = s[t];
  if (rho3) { const Rho3 r = loss_eval<LM>(loss, sq); rho3[3 * t] = r.r0; rho3[3 * t + 1] = r.r1; rho3[3 * t + 2] = r.r2; }
  if (val) val[t] = loss_value<LM>(loss, sq);
  if (LM != LM_PROGRAM && rho1) rho1[t] = loss_rho1<LM>(loss, sq);
}

// out[0] = sum partials (single block, fixed order)
__global__ void __launch_bounds__(GSFM_BLOCK) k_sum_partials(const double* __restrict__ partials, int n, double* out) {
  __shared__ double lds[8];
  const double t = sum_partials_bcast(partials, n, lds);
  if (threadIdx.x == 0) out[0] = t;
}

}  // namespace gsfm
