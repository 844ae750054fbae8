// K3: the row-major normal-equation mat-vec, MatvecArgs and k_matvec.  Launched by launch_matvec in solver_launch.hpp; the fused PCG
// form k_matvec_cg (pcg_kernels.hpp) takes the same arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"

namespace gsfm {

#ifndef GSFM_GATHER_LOAD
#define GSFM_GATHER_LOAD(p) (*(p))   // tuning hook: e.g. __builtin_nontemporal_load(p)
#endif

// ------------------------------------------------------------------------------------------
// K3: y_k = M_k p_k + sum_d H_d p[col_d]   (M = diagonal block incl. LM damping, sym 6)
// ------------------------------------------------------------------------------------------
struct MatvecArgs {
  uint32_t n_rows, row_base, G;
  const uint32_t* row_ptr;
  const uint32_t* col;
  const double2 *h0, *h1, *h2, *h3;
  const double* h4;
  const double* Mblk;   // 6 per camera
  const double* p;      // 3 per camera
  double* y;            // 3 per camera
  const int* done;      // PCG convergence flag (may be null)
  const double2* q;     // LAP: camera quaternions
  const double* u;      // LAP: u_k = R_k^T p_k, 3 per camera
};
// LAP = false: y_k = M_k p_k + sum_d H_d p[col_d], 76 B per entry.  LAP = true: y_k = M_k p_k - sum_d G_d (R_k u[col_d]), 52 B per entry.
template <bool LAP>
__global__ void __launch_bounds__(GSFM_BLOCK) k_matvec(MatvecArgs a) {
  if (a.done && *a.done) return;
  const uint32_t G = a.G;
  const uint32_t t = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const uint32_t row = t / G, lane = t % G;
  const bool live = row < a.n_rows;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  if (live) {
    double Rk[9];
    if (LAP) qmat(load_q(a.q, a.row_base + row), Rk);
    const uint32_t end = a.row_ptr[row + 1];
    for (uint32_t d = a.row_ptr[row] + lane; d < end; d += G) {
      const uint32_t m = __builtin_nontemporal_load(a.col + d) & 0x7fffffffu;
      // the blocks are streamed once per mat-vec: non-temporal loads keep the gathered vector resident in L2
      if (LAP) {
        const double2 A = nt_load2(a.h0 + d), B = nt_load2(a.h1 + d), C = nt_load2(a.h2 + d);   // (g00 g01) (g02 g11) (g12 g22)
        const double* um = a.u + 3 * (size_t)m;
        const double u0 = GSFM_GATHER_LOAD(um), u1 = GSFM_GATHER_LOAD(um + 1), u2 = GSFM_GATHER_LOAD(um + 2);
        const double w0 = Rk[0] * u0 + Rk[1] * u1 + Rk[2] * u2, w1 = Rk[3] * u0 + Rk[4] * u1 + Rk[5] * u2, w2 = Rk[6] * u0 + Rk[7] * u1 + Rk[8] * u2;
        y0 += A.x * w0 + A.y * w1 + B.x * w2;
        y1 += A.y * w0 + B.y * w1 + C.x * w2;
        y2 += B.x * w0 + C.x * w1 + C.y * w2;
      } else {
        const double2 A = nt_load2(a.h0 + d), B = nt_load2(a.h1 + d), C = nt_load2(a.h2 + d), D = nt_load2(a.h3 + d);
        const double E = __builtin_nontemporal_load(a.h4 + d);
        const double* pm = a.p + 3 * (size_t)m;
        const double p0 = pm[0], p1 = pm[1], p2 = pm[2];
        y0 += A.x * p0 + A.y * p1 + B.x * p2;
        y1 += B.y * p0 + C.x * p1 + C.y * p2;
        y2 += D.x * p0 + D.y * p1 + E * p2;
      }
    }
  }
  for (uint32_t off = G >> 1; off > 0; off >>= 1) {
    y0 += __shfl_down(y0, off, G); y1 += __shfl_down(y1, off, G); y2 += __shfl_down(y2, off, G);
  }
  if (live && lane == 0) {
    const size_t k = a.row_base + row;
    const double* M = a.Mblk + 6 * k;
    const double* pk = a.p + 3 * k;
    double mp[3];
    sym3_mulvec(M, pk, mp);
    const double sgn = LAP ? -1.0 : 1.0;
    a.y[3 * k] = mp[0] + sgn * y0; a.y[3 * k + 1] = mp[1] + sgn * y1; a.y[3 * k + 2] = mp[2] + sgn * y2;
  }
}

}  // namespace gsfm
