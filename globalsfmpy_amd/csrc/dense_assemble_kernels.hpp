// Dense assembly for the exact Cholesky step: DenseArgs, the dense-entry helpers (dense_elem, dense_entry_block, dense_pair_sum) and
// k_dense_assemble.  Launched by run_dense in solver_dense.hpp; the helpers are shared with comp_kernels.hpp and colsort_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"

namespace gsfm {

// ------------------------------------------------------------------------------------------
// Small graphs: assemble the damped normal matrix for the exact Cholesky step (dense_kernels.hpp) -- lower triangle only,
// as 32 x 32 tiles, plus the right-hand side -g as block row T.  The block-CSR holds both directions of every edge; the
// lower triangle takes the entry whose row camera has the larger index (H_km for k > m).  A camera pair measured several times
// has several entries (m, in either orientation) in row k, in edge order but not adjacent: the lane of the FIRST of them adds
// all of them in CSR order, from +0.0, and writes the cell once; the others skip.  So the cell never depends on which lane or
// wavefront runs first (fp64 atomics would: three or more addends do not commute in floating point), and for one or two
// entries it is the sum the zero-filled cell and atomicAdd gave (0 + a; a + b = b + a).  A is zero-filled before the launch.
// ------------------------------------------------------------------------------------------
struct DenseArgs {
  uint32_t n_rows;
  const uint32_t* row_ptr;
  const uint32_t* col;
  const double2 *h0, *h1, *h2, *h3;
  const double* h4;
  const double* Mblk;  // 6 per camera
  const double* b;     // 3 per camera: right-hand side
  double* A;           // tiles, see chol_tile_off
  uint32_t n, T;
  const double2* q;    // Laplacian form (lap = 1): planes h0..h2 hold G_k, the block is -G_k R_k R_m^T
  int lap;
  double* info_slot;   // status word of the factorisation (an int in a double slot of the scalar block) and
  double* rcg;         // the PCG residual (3 per camera, zero for an exact solve): cleared here instead of by two more memset nodes
};
__device__ __forceinline__ double* dense_elem(double* A, uint32_t gr, uint32_t gc) {
  return A + ((size_t)(gr / 32) * (gr / 32 + 1) / 2 + gc / 32) * 1024 + (gr % 32) * 32 + gc % 32;
}
// the off-diagonal block of directed entry d (row camera `row`, neighbour m) as the layout stores it, or rebuilt from the Laplacian form
__device__ __forceinline__ void dense_entry_block(const DenseArgs& a, uint32_t row, uint32_t m, uint32_t d, double* H) {
  if (a.lap) {
    const double2 A0 = a.h0[d], B0 = a.h1[d], C0 = a.h2[d];
    const double Gm[9] = {A0.x, A0.y, B0.x, A0.y, B0.y, C0.x, B0.x, C0.x, C0.y};
    double Rk[9], Rm[9], T[9];
    qmat(load_q(a.q, row), Rk);
    qmat(load_q(a.q, m), Rm);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T[3 * r + c] = Rk[3 * r] * Rm[3 * c] + Rk[3 * r + 1] * Rm[3 * c + 1] + Rk[3 * r + 2] * Rm[3 * c + 2];   // R_k R_m^T
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[3 * r + c] = -(Gm[3 * r] * T[c] + Gm[3 * r + 1] * T[3 + c] + Gm[3 * r + 2] * T[6 + c]);
  } else {
    const double2 A0 = a.h0[d], B0 = a.h1[d], C0 = a.h2[d], D0 = a.h3[d];
    H[0] = A0.x; H[1] = A0.y; H[2] = B0.x; H[3] = B0.y; H[4] = C0.x; H[5] = C0.y; H[6] = D0.x; H[7] = D0.y; H[8] = a.h4[d];
  }
}
// Row-major block-CSR, row `row` (entries a.row_ptr[lrow] ..): false if an earlier entry of the row has neighbour m (its lane writes the cell);
// else S = +0.0 + the blocks of all of the row's entries with neighbour m, in CSR order.  The scan is uniform over the row (broadcast loads
// of `col`); only a repeated pair takes the second loop.  Cost: deg reads of `col` per lower-triangle entry, O(deg^2) per row where the
// atomics were O(deg) -- deg / 256 trips of a deg-long loop per lane, on a row the L1 holds; the exact step serves graphs of a few thousand
// cameras at most (dense_cholesky_auto_cams), and the benchmark's exact-step graphs (Madrid, C4) time the same as with the atomics.
__device__ __forceinline__ bool dense_pair_sum(const DenseArgs& a, uint32_t row, uint32_t m, uint32_t d, double* S, uint32_t lrow) {
  const uint32_t d0 = a.row_ptr[lrow], d1 = a.row_ptr[lrow + 1];
  bool first = true, more = false;
  for (uint32_t e = d0; e < d1; ++e) {
    const bool same = (a.col[e] & 0x7fffffffu) == m;
    first = first && !(same && e < d);
    more = more || (same && e > d);
  }
  if (!first) return false;
  double H[9];
  dense_entry_block(a, row, m, d, H);
  for (int k = 0; k < 9; ++k) S[k] = 0.0 + H[k];
  if (more)
    for (uint32_t e = d + 1; e < d1; ++e) {
      if ((a.col[e] & 0x7fffffffu) != m) continue;
      dense_entry_block(a, row, m, e, H);
      for (int k = 0; k < 9; ++k) S[k] += H[k];
    }
  return true;
}
__device__ __forceinline__ bool dense_pair_sum(const DenseArgs& a, uint32_t row, uint32_t m, uint32_t d, double* S) { return dense_pair_sum(a, row, m, d, S, row); }
__global__ void __launch_bounds__(GSFM_BLOCK) k_dense_assemble(DenseArgs a) {
  const uint32_t row = blockIdx.x;
  if (row >= a.n_rows) return;
  if (threadIdx.x < 3) a.rcg[3 * (size_t)row + threadIdx.x] = 0.0;
  if (row == 0 && threadIdx.x == 3) *a.info_slot = 0.0;
  if (threadIdx.x == 0) {
    const double* M = a.Mblk + 6 * (size_t)row;
    const double m[9] = {M[0], M[1], M[2], M[1], M[3], M[4], M[2], M[4], M[5]};
    for (int r = 0; r < 3; ++r) for (int c = 0; c <= r; ++c) *dense_elem(a.A, 3 * row + r, 3 * row + c) = m[3 * r + c];
    for (int c = 0; c < 3; ++c) a.A[(((size_t)a.T * (a.T + 1) / 2) + (3 * row + c) / 32) * 1024 + (3 * row + c) % 32] = a.b[3 * (size_t)row + c];
    if (row == 0) for (uint32_t g = a.n; g < a.T * 32; ++g) *dense_elem(a.A, g, g) = 1.0;   // padding of the last tile: identity
  }
  for (uint32_t d = a.row_ptr[row] + threadIdx.x; d < a.row_ptr[row + 1]; d += GSFM_BLOCK) {
    const uint32_t m = a.col[d] & 0x7fffffffu;
    if (m >= row) continue;   // upper triangle (and self loops, which cannot occur)
    double H[9];
    if (!dense_pair_sum(a, row, m, d, H)) continue;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) *dense_elem(a.A, 3 * row + r, 3 * m + c) = H[3 * r + c];
  }
}

}  // namespace gsfm
