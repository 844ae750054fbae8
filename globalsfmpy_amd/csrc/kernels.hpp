// HIP kernels of the rotation-averaging hot path (gfx950, fp64, HBM-bound; no MFMA: there is
// no dense contraction on this path).
//
// Data layout in HBM (all per-edge streams are planes of 16-byte chunks so that a wavefront's
// loads are 64 x 16 B = 1 KiB contiguous):
//   cameras        quats  q[k]  = 2 x double2 (x,y)(z,w)     gathered (L2 / Infinity-Cache resident)
//   cost edges     idx    uint2 (i, j)                        8 B / edge
//                  qrel   2 planes of double2                 32 B / edge
//                  W      0 | 1 plane double | 3 planes double2 (upper-triangular Lt) 0 / 8 / 48 B
//   directed rows  one entry per (owned camera k <- neighbour m) = the block-CSR structure of
//                  J^T J; per entry: col (u32, bit31 = role), qrel, W (copies), H block (72 B,
//                  4 planes double2 + 1 plane double) written by K2, read by K3.
//
// One header per kernel family, in the order the text reaches the library:
//   edge_math.hpp               reductions, EdgeW, edge_residual / edge_linearize, robustify, plane loads, the qrel 3/4-component coding
//   setup_kernels.hpp       K0  k_build_qrel, k_whiten, sigma consensus, k_edge_sweep, k_row_s, k_gather_weights
//   cost_kernels.hpp        K1  k_cost      1 edge / lane            residual + robust reweight sweep, block-reduced cost
//   lin_kernels.hpp         K2  k_lin       G lanes / camera row     residual, 3x3 body Jacobians, Corrector, g, D, H blocks
//   matvec_kernels.hpp      K3  k_matvec    G lanes / camera row     y = M p + sum_d H_d p[col_d]
//   cam_kernels.hpp         K5  k_cam_*     1 camera / lane          quaternion cache, LM diagonal / preconditioner, step
//   pcg_kernels.hpp         K4  k_cg_*      1 camera / lane          fused PCG vector updates + dot-product partials; coarse level, mailbox, k_matvec_cg
//   dense_assemble_kernels.hpp  DenseArgs, k_dense_assemble          the damped normal matrix as tiles for the exact Cholesky step (dense_kernels.hpp)
//   lm_kernels.hpp              LmOpts, k_lm_decide, k_lm_after      device-side LM control for exact steps
// (K2c / K3c, the column-sorted forms, are in colsort_kernels.hpp; the batched small-component kernels in comp_kernels.hpp.)
#pragma once
#include "edge_math.hpp"
#include "setup_kernels.hpp"
#include "cost_kernels.hpp"
#include "lin_kernels.hpp"
#include "matvec_kernels.hpp"
#include "cam_kernels.hpp"
#include "pcg_kernels.hpp"
#include "dense_assemble_kernels.hpp"
#include "lm_kernels.hpp"
