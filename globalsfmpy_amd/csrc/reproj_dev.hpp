// The reprojection residual of one observation with fixed orientation, its 2 x 3 point Jacobian and Ceres' Corrector: the device routine
// shared by the per-track refinement (track_refine_kernels.hpp, trr_pass) and the bundle adjustment of positions and points
// (ba_kernels.hpp).  One text, so that both evaluate an observation with the same rounding.
//   cam     a camera record of k_tri_cameras (triangulate_kernels.hpp): R row-major (9), position (3, not read here), f u v, estimated
//   v       X - o, the point relative to the camera centre;  p = R v
//   r       (f p_x / p_z + u - x, f p_y / p_z + v - y),  s = |r|^2
//   J       (f / p_z) [[1, 0, -p_x / p_z], [0, 1, -p_y / p_z]] R: the Jacobian with respect to the point (minus that with respect to o)
//   Corrector (corrector.cc of Ceres 1.14): J <- sqrt(rho') (J - alpha / s r r^T J), r <- sqrt(rho') / (1 - alpha) r
#pragma once
#include <hip/hip_runtime.h>
#include "loss_dev.hpp"

namespace gsfm {

// the plain residual (ex, ey) of an observation
__device__ __forceinline__ void reproj_residual(const double* cam, double2 xy, double v0, double v1, double v2, double& ex, double& ey) {
  const double px = cam[0] * v0 + cam[1] * v1 + cam[2] * v2, py = cam[3] * v0 + cam[4] * v1 + cam[5] * v2, pz = cam[6] * v0 + cam[7] * v1 + cam[8] * v2;
  ex = cam[12] * px / pz + cam[13] - xy.x; ey = cam[12] * py / pz + cam[14] - xy.y;
}

// the corrected Jacobian rows J0, J1, the corrected residual (r0, r1) and rho(s)
__device__ __forceinline__ void reproj_corrected(const double* cam, double2 xy, double v0, double v1, double v2, const DevLossNode& leaf, double* J0, double* J1,
                                                 double& r0, double& r1, double& rho0) {
  const double px = cam[0] * v0 + cam[1] * v1 + cam[2] * v2, py = cam[3] * v0 + cam[4] * v1 + cam[5] * v2, pz = cam[6] * v0 + cam[7] * v1 + cam[8] * v2;
  const double ex = cam[12] * px / pz + cam[13] - xy.x, ey = cam[12] * py / pz + cam[14] - xy.y;
  const double sq = ex * ex + ey * ey;
  const Rho3 rho = loss_leaf_simple(leaf, sq);
  const Corrector c = make_corrector(sq, rho);
  const double fz = cam[12] / pz, ax = px / pz, ay = py / pz;
#pragma unroll
  for (int j = 0; j < 3; ++j) { J0[j] = fz * (cam[j] - ax * cam[6 + j]); J1[j] = fz * (cam[3 + j] - ay * cam[6 + j]); }
  if (c.alpha_sq_norm != 0.0) {                      // Corrector::CorrectJacobian: J <- J - alpha / s r r^T J
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double t = c.alpha_sq_norm * (ex * J0[j] + ey * J1[j]);
      J0[j] -= ex * t; J1[j] -= ey * t;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { J0[j] *= c.sqrt_rho1; J1[j] *= c.sqrt_rho1; }
  r0 = c.residual_scaling * ex; r1 = c.residual_scaling * ey;
  rho0 = rho.r0;
}

// reproj_corrected with a free orientation (full_ba_kernels.hpp): also the corrected 2 x 3 Jacobian with respect to the angle-axis vector w,
// Jr = -P [p]x J_l(w) with P = (f / p_z) [[1, 0, -p_x / p_z], [0, 1, -p_y / p_z]].  Row i of -P [p]x is p x P_i; Jl is J_l(w), row-major.
// WITH_F (a free focal length): also the corrected Jacobian with respect to f, Jf = (p_x / p_z, p_y / p_z), one entry per residual row;
// without it Jf is not touched.  The residual, the loss and the point rows J0, J1 are computed by the text of reproj_corrected (the same
// rounding), and one text serves both settings of WITH_F; the Corrector mixes the two rows of Jr and the two entries of Jf exactly as it mixes
// the rows of the point Jacobian.
template <bool WITH_F>
__device__ __forceinline__ void reproj_corrected_free(const double* cam, const double* Jl, double2 xy, double v0, double v1, double v2, const DevLossNode& leaf,
                                                      double* J0, double* J1, double* Jr0, double* Jr1, double* Jf, double& r0, double& r1, double& rho0) {
  const double px = cam[0] * v0 + cam[1] * v1 + cam[2] * v2, py = cam[3] * v0 + cam[4] * v1 + cam[5] * v2, pz = cam[6] * v0 + cam[7] * v1 + cam[8] * v2;
  const double ex = cam[12] * px / pz + cam[13] - xy.x, ey = cam[12] * py / pz + cam[14] - xy.y;
  const double sq = ex * ex + ey * ey;
  const Rho3 rho = loss_leaf_simple(leaf, sq);
  const Corrector c = make_corrector(sq, rho);
  const double fz = cam[12] / pz, ax = px / pz, ay = py / pz;
#pragma unroll
  for (int j = 0; j < 3; ++j) { J0[j] = fz * (cam[j] - ax * cam[6 + j]); J1[j] = fz * (cam[3 + j] - ay * cam[6 + j]); }
  // p x P_0 with P_0 = fz (1, 0, -ax), p x P_1 with P_1 = fz (0, 1, -ay)
  const double c0[3] = {fz * (-py * ax), fz * (pz + px * ax), fz * (-py)};
  const double c1[3] = {fz * (-py * ay - pz), fz * (px * ay), fz * px};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    Jr0[j] = c0[0] * Jl[j] + c0[1] * Jl[3 + j] + c0[2] * Jl[6 + j];
    Jr1[j] = c1[0] * Jl[j] + c1[1] * Jl[3 + j] + c1[2] * Jl[6 + j];
  }
  if constexpr (WITH_F) { Jf[0] = ax; Jf[1] = ay; }
  if (c.alpha_sq_norm != 0.0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double t = c.alpha_sq_norm * (ex * J0[j] + ey * J1[j]);
      J0[j] -= ex * t; J1[j] -= ey * t;
      const double tr = c.alpha_sq_norm * (ex * Jr0[j] + ey * Jr1[j]);
      Jr0[j] -= ex * tr; Jr1[j] -= ey * tr;
    }
    if constexpr (WITH_F) {
      const double tf = c.alpha_sq_norm * (ex * Jf[0] + ey * Jf[1]);
      Jf[0] -= ex * tf; Jf[1] -= ey * tf;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { J0[j] *= c.sqrt_rho1; J1[j] *= c.sqrt_rho1; Jr0[j] *= c.sqrt_rho1; Jr1[j] *= c.sqrt_rho1; }
  if constexpr (WITH_F) { Jf[0] *= c.sqrt_rho1; Jf[1] *= c.sqrt_rho1; }
  r0 = c.residual_scaling * ex; r1 = c.residual_scaling * ey;
  rho0 = rho.r0;
}

}  // namespace gsfm
