// Device side of the robust L1 + IRLS rotation estimator (include/gsfm_rot_l1l2.h; host side rot_l1l2.hpp).  fp64 throughout.
//   k_l1_setup        rotations and measurements as unit quaternions (so3_dev.hpp), once per call
//   k_l1_resid        edge sweep: b_e = Log(R_j^T R_ij R_i), |b_e|^2, the IRLS weight w_e, w_e b_e, and w_e at the edge's two directed entries
//   k_l1_admm_edge    one per ADMM iteration: A x from x, z and u in place, the next right-hand side vector b + z - u, z - z_old, and the
//                     partial sums of |A x - z - b|^2, |A x|^2, |z|^2, |b|^2
//   k_l1_rows<NV, G>  one per ADMM iteration (NV = 3) and per IRLS iteration (NV = 1): A^T of NV edge vectors per free camera, gathered
//                     along the camera's row; NV = 3 also sums |rho A^T (z - z_old)|^2 and |rho A^T u|^2, NV = 1 the weighted degree
//   k_l1_matvec<W, G> y_k = d_k p_k - sum_m w_km p_m with the partial sums of p.y; W = false reads no weight: 4 B per directed entry
//                     (the neighbour) against 12 B weighted
//   k_l1_pcg_*        the PCG vector updates with their dot-product partials;  k_l1_reduce: the partials of a launch into device scalars
//   k_l1_update       R_k <- R_k Exp(x_k) on the free cameras, the partial sums of |x_k|;  k_l1_finish: quaternions back to angle-axis
//   k_l1_post         the host's look at the device scalars: mapped host memory, the stamp last
// Rows.  A free camera's row is handled by a group of G lanes: G = 8 for rows of up to L1_SHORT_ROW entries, a whole wavefront (G = 64) for
// longer ones -- two launches over two row lists (rot_l1l2_structure.hpp), so that a hub of thousands of entries costs its wavefront
// len / 64 steps while the lanes beside a short row are not idle for them.  Lane l of a group adds the entries l, l + G, ... in order,
// then an xor butterfly over the group: the order of every sum is a function of the row alone.
// Reductions.  Every launch writes one partial per workgroup; k_l1_reduce adds them in index order.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"
#include "so3_dev.hpp"

namespace gsfm {

#define GSFM_L1_MAX_BLOCKS 1024   // workgroups of the strided edge and vector kernels: at most so many partials per sum

// device scalars of a call (the first three are lm_loop.hpp's PCG_RZ0 / PCG_RZA / PCG_RZB)
enum { L1S_RZ0 = 0, L1S_RZA = 1, L1S_RZB = 2, L1S_PAP = 3, L1S_R2 = 4, L1S_AX2 = 5, L1S_Z2 = 6, L1S_B2 = 7, L1S_S2 = 8, L1S_ATU2 = 9, L1S_STEP = 10, L1S_N = 11 };

__global__ void __launch_bounds__(256) k_l1_setup(uint32_t n_cams, uint32_t n_edges, const double* __restrict__ rot_aa, const double* __restrict__ rel_aa,
                                                  Quat* __restrict__ q, Quat* __restrict__ qrel) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_cams) q[t] = aa_to_quat(rot_aa[3 * t], rot_aa[3 * t + 1], rot_aa[3 * t + 2]);
  if (t < n_edges) qrel[t] = aa_to_quat(rel_aa[3 * t], rel_aa[3 * t + 1], rel_aa[3 * t + 2]);
}

// b, sq, w, wb: per edge, each may be NULL; wd: per directed entry (with pos_i / pos_j), may be NULL
__global__ void __launch_bounds__(256) k_l1_resid(uint32_t n_edges, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej, const Quat* __restrict__ q,
                                                  const Quat* __restrict__ qrel, double sigma, const uint32_t* __restrict__ pos_i,
                                                  const uint32_t* __restrict__ pos_j, double* __restrict__ b, double* __restrict__ sq, double* __restrict__ w,
                                                  double* __restrict__ wb, double* __restrict__ wd) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  const Quat err = qmul(qconj(q[ej[e]]), qmul(qrel[e], q[ei[e]]));
  double r[3], s, theta;
  quat_log(err, r, &s, &theta);
  const double s2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const double t = s2 + sigma * sigma;
  const double we = sigma / (t * t);
  if (b) { b[3 * e] = r[0]; b[3 * e + 1] = r[1]; b[3 * e + 2] = r[2]; }
  if (sq) sq[e] = s2;
  if (w) w[e] = we;
  if (wb) { wb[3 * e] = we * r[0]; wb[3 * e + 1] = we * r[1]; wb[3 * e + 2] = we * r[2]; }
  if (wd) { wd[pos_i[e]] = we; wd[pos_j[e]] = we; }
}

// the edge weights of the Laplacian aid at the edges' directed entries
__global__ void __launch_bounds__(256) k_l1_spread(uint32_t n_edges, const double* __restrict__ w, const uint32_t* __restrict__ pos_i,
                                                   const uint32_t* __restrict__ pos_j, double* __restrict__ wd) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  wd[pos_i[e]] = w[e]; wd[pos_j[e]] = w[e];
}

// x is zero on the fixed camera (and on every camera without an edge), so (A x)_e = x_j - x_i needs no mask.
// part: four planes, `stride` apart, of gridDim.x partials (|A x - z - b|^2, |A x|^2, |z|^2, |b|^2)
__global__ void __launch_bounds__(256) k_l1_admm_edge(uint32_t n_edges, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej, const double* __restrict__ x,
                                                      const double* __restrict__ b, double* __restrict__ z, double* __restrict__ u, double* __restrict__ v,
                                                      double* __restrict__ dz, double rho, double alpha, double* __restrict__ part, uint32_t stride) {
  __shared__ double lds[5];
  const double kappa = 1.0 / rho;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (size_t)gridDim.x * 256) {
    const size_t i3 = 3 * (size_t)ei[e], j3 = 3 * (size_t)ej[e];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t t = 3 * e + c;
      const double ax = x[j3 + c] - x[i3 + c], bb = b[t], zo = z[t], uo = u[t];
      const double h = alpha * ax + (1.0 - alpha) * (zo + bb);
      const double a = h - bb + uo;
      const double zn = fmax(0.0, a - kappa) - fmax(0.0, -a - kappa);
      const double un = uo + (h - zn - bb);
      z[t] = zn; u[t] = un; v[t] = bb + zn - un; dz[t] = zn - zo;
      const double rr = ax - zn - bb;
      acc[0] += rr * rr; acc[1] += ax * ax; acc[2] += zn * zn; acc[3] += bb * bb;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = block_sum_bcast(acc[k], lds);
    if (threadIdx.x == 0) part[(size_t)k * stride + blockIdx.x] = t;
  }
}

template <int G> __device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Group g of G lanes gathers row rows[g]: out0_k = sum over the row's entries of +-v0_e (the sign of A^T: + at the edge's j end).
// NV = 3: the same sums of v1 and v2 stay in registers and their squared norms, times rho^2, go to part[blk] and part[stride + blk]
// (blk = part_off + blockIdx.x).  NV = 1: with wd the row's weights are summed into deg_k.
template <int NV, int G>
__global__ void __launch_bounds__(256) k_l1_rows(const uint32_t* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ row_ptr,
                                                 const uint32_t* __restrict__ ent, const double* __restrict__ v0, const double* __restrict__ v1,
                                                 const double* __restrict__ v2, const double* __restrict__ wd, double* __restrict__ out0,
                                                 double* __restrict__ deg, double rho, double* __restrict__ part, uint32_t part_off, uint32_t stride) {
  __shared__ double lds[5];
  const uint32_t g = (blockIdx.x * 256 + threadIdx.x) / G, lane = threadIdx.x % G;
  const bool live = g < n_rows;
  const uint32_t k = live ? rows[g] : 0u;
  const uint32_t beg = live ? row_ptr[k] : 0u, end = live ? row_ptr[k + 1] : 0u;
  double s[3 * NV], dsum = 0.0;
#pragma unroll
  for (int c = 0; c < 3 * NV; ++c) s[c] = 0.0;
  for (uint32_t d = beg + lane; d < end; d += G) {
    const uint32_t en = ent[d];
    const size_t e3 = 3 * (size_t)(en >> 1);
    const double sg = (en & 1u) ? 1.0 : -1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[c] += sg * v0[e3 + c];
      if (NV == 3) { s[3 + c] += sg * v1[e3 + c]; s[6 + c] += sg * v2[e3 + c]; }
    }
    if (NV == 1 && wd) dsum += wd[d];
  }
#pragma unroll
  for (int c = 0; c < 3 * NV; ++c) s[c] = group_sum<G>(s[c]);
  if (NV == 1 && wd) dsum = group_sum<G>(dsum);
  if (live && lane == 0) {
    out0[3 * (size_t)k] = s[0]; out0[3 * (size_t)k + 1] = s[1]; out0[3 * (size_t)k + 2] = s[2];
    if (NV == 1 && wd) deg[k] = dsum;
  }
  if (NV == 3) {
    const bool mine = live && lane == 0;
    const double a = mine ? rho * rho * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]) : 0.0;
    const double c = mine ? rho * rho * (s[6] * s[6] + s[7] * s[7] + s[8] * s[8]) : 0.0;
    const double ta = block_sum_bcast(a, lds);
    const double tc = block_sum_bcast(c, lds);
    if (threadIdx.x == 0) { part[part_off + blockIdx.x] = ta; part[(size_t)stride + part_off + blockIdx.x] = tc; }
  }
}

// y_k = d_k p_k - sum over the row's entries of w p_nbr on the free rows (p is zero on every other camera, y is never written there), and
// the partials of p.y at part[part_off + blockIdx.x]
template <bool W, int G>
__global__ void __launch_bounds__(256) k_l1_matvec(const uint32_t* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ row_ptr,
                                                   const uint32_t* __restrict__ nbr, const double* __restrict__ wd, const double* __restrict__ deg,
                                                   const double* __restrict__ p, double* __restrict__ y, double* __restrict__ part, uint32_t part_off) {
  __shared__ double lds[5];
  const uint32_t g = (blockIdx.x * 256 + threadIdx.x) / G, lane = threadIdx.x % G;
  const bool live = g < n_rows;
  const uint32_t k = live ? rows[g] : 0u;
  const uint32_t beg = live ? row_ptr[k] : 0u, end = live ? row_ptr[k + 1] : 0u;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (uint32_t d = beg + lane; d < end; d += G) {
    const size_t m3 = 3 * (size_t)nbr[d];
    if (W) { const double w = wd[d]; s0 += w * p[m3]; s1 += w * p[m3 + 1]; s2 += w * p[m3 + 2]; }
    else { s0 += p[m3]; s1 += p[m3 + 1]; s2 += p[m3 + 2]; }
  }
  s0 = group_sum<G>(s0); s1 = group_sum<G>(s1); s2 = group_sum<G>(s2);
  double dot = 0.0;
  if (live && lane == 0) {
    const size_t k3 = 3 * (size_t)k;
    const double dk = deg[k], p0 = p[k3], p1 = p[k3 + 1], p2 = p[k3 + 2];
    const double y0 = dk * p0 - s0, y1 = dk * p1 - s1, y2 = dk * p2 - s2;
    y[k3] = y0; y[k3 + 1] = y1; y[k3 + 2] = y2;
    dot = p0 * y0 + p1 * y1 + p2 * y2;
  }
  const double t = block_sum_bcast(dot, lds);
  if (threadIdx.x == 0) part[part_off + blockIdx.x] = t;
}

// out[c] = the sum of plane c's n partials in index order, c < m (planes `stride` apart); one workgroup
__global__ void __launch_bounds__(256) k_l1_reduce(const double* __restrict__ part, uint32_t n, uint32_t stride, int m, double* __restrict__ out) {
  __shared__ double lds[5];
  for (int c = 0; c < m; ++c) {
    double acc = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += 256) acc += part[(size_t)c * stride + k];
    const double t = block_sum_bcast(acc, lds);
    if (threadIdx.x == 0) out[c] = t;
  }
}

// PCG from y = 0 over the n3 = 3 n_cams entries: r = rhs, z = r / d, p = z, the partials of r.z.  rhs is zero off the free cameras and d
// is 1 there, so every vector stays zero there.
__global__ void __launch_bounds__(256) k_l1_pcg_start(size_t n3, const double* __restrict__ rhs, const double* __restrict__ deg, double* __restrict__ r,
                                                      double* __restrict__ z, double* __restrict__ p, double* __restrict__ y, double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (size_t)gridDim.x * 256) {
    const double ri = rhs[i], zi = ri / deg[i / 3];
    r[i] = ri; z[i] = zi; p[i] = zi; y[i] = 0.0;
    acc += ri * zi;
  }
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// y += alpha p, r -= alpha A p, z = r / d with alpha = rz / pAp from the device scalars; the partials of the new r.z
__global__ void __launch_bounds__(256) k_l1_pcg_update(size_t n3, const double* __restrict__ scal, int s_rz, const double* __restrict__ p,
                                                       const double* __restrict__ Ap, const double* __restrict__ deg, double* __restrict__ y,
                                                       double* __restrict__ r, double* __restrict__ z, double* __restrict__ part) {
  __shared__ double lds[5];
  const double pap = scal[L1S_PAP];
  const double alpha = pap > 0.0 ? scal[s_rz] / pap : 0.0;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (size_t)gridDim.x * 256) {
    y[i] += alpha * p[i];
    const double ri = r[i] - alpha * Ap[i], zi = ri / deg[i / 3];
    r[i] = ri; z[i] = zi;
    acc += ri * zi;
  }
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// p = z + beta p, beta = rz_new / rz
__global__ void __launch_bounds__(256) k_l1_pcg_dir(size_t n3, const double* __restrict__ scal, int s_rzn, int s_rz, const double* __restrict__ z,
                                                    double* __restrict__ p) {
  const double rz = scal[s_rz];
  const double beta = rz > 0.0 ? scal[s_rzn] / rz : 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (size_t)gridDim.x * 256) p[i] = z[i] + beta * p[i];
}

// R_k <- R_k Exp(x_k) on the free cameras (renormalised: up to 105 products follow each other), touched_k set by a step that is not
// exactly zero, and the partials of sum |x_k|
__global__ void __launch_bounds__(256) k_l1_update(uint32_t n_cams, const uint8_t* __restrict__ active, const double* __restrict__ x, Quat* __restrict__ q,
                                                   uint8_t* __restrict__ touched, double* __restrict__ part) {
  __shared__ double lds[5];
  double acc = 0.0;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n_cams; k += (size_t)gridDim.x * 256) {
    if (!active[k]) continue;
    const double x0 = x[3 * k], x1 = x[3 * k + 1], x2 = x[3 * k + 2];
    const double n = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
    acc += n;
    if (n > 0.0) {
      Quat r = qmul(q[k], aa_to_quat(x0, x1, x2));
      const double inv = 1.0 / sqrt(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
      r.x *= inv; r.y *= inv; r.z *= inv; r.w *= inv;
      q[k] = r;
      touched[k] = 1;
    }
  }
  const double t = block_sum_bcast(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// the rotations of the touched cameras back to angle-axis (Ceres' QuaternionToAngleAxis); every other camera keeps its input
__global__ void __launch_bounds__(256) k_l1_finish(uint32_t n_cams, const Quat* __restrict__ q, const uint8_t* __restrict__ touched, double* __restrict__ rot_aa) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cams || !touched[k]) return;
  double e[3], s, theta;
  quat_log(q[k], e, &s, &theta);
  rot_aa[3 * k] = e[0]; rot_aa[3 * k + 1] = e[1]; rot_aa[3 * k + 2] = e[2];
}

// the host's look: n device scalars to mapped host memory, the stamp after them
__global__ void k_l1_post(const double* __restrict__ scal, int n, double* mail, unsigned long long* stamp_word, unsigned long long stamp) {
  for (int k = 0; k < n; ++k) mail[k] = scal[k];
  __hip_atomic_store(stamp_word, stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace gsfm
