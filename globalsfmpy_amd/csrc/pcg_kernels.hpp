// K4: both PCG recurrences -- the classic vector kernels (CgScalars, CgArgs, k_cg_*), the coarse level (CoarseArgs, k_coarse_*), and the
// single-reduction recurrence with its host mailbox (Cg2Scalars, Cg2Args, k_cg2_*, k_matvec_cg).  Launched by solver_pcg.hpp; Cg2Args is
// shared with the column-sorted k_mv_col_cg (colsort_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"
#include "matvec_kernels.hpp"
#include "cam_kernels.hpp"

namespace gsfm {

// ------------------------------------------------------------------------------------------
// K4: PCG vector kernels.  Device scalars: rz[2] (parity-indexed), rz0, done, iters.
// ------------------------------------------------------------------------------------------
struct CgScalars {
  double rz[2];
  double rz0;
  double last_rel;  // sqrt(rz/rz0) at the last iteration
  double best_rel;  // smallest relative residual seen so far (stagnation detection)
  int done;
  int iters;
  int stall;        // iterations since best_rel last halved
  int stalled;      // 1 if the solve ended by stagnation
  int done_seen;    // `done` as k_cg_update found it: what k_cg_pupdate -- the kernel that SETS done -- tests at its entry, so that the launch that
                    // detects convergence still updates p on every block and leaves a state the solve can be resumed from (k_cg_resume)
  int pad_;
  double tol;       // relative tolerance of the current run: device-resident, so that a captured chunk does not freeze it (forcing schedule,
                    // solver_lm.hpp: a loose solve may be continued to the tight tolerance, bit for bit as if it had never stopped)
  double etol2;     // loose solves: stop once the ESTIMATED relative energy-norm error of the iterate, squared, is below this (0 = off); see cg_energy_stop
  double esum;      // sum of the iterations' decreases of the quadratic model, alpha_j (r_j . z_j) = |x_{j+1}|_A^2 - |x_j|_A^2 growth (Hestenes-Stiefel)
  double einc[4];   // the last four of them (ring, indexed by iteration & 3)
  double rz_abs;    // absolute floor on r.z (k_cam_bound): `tol` never drops below sqrt(rz_abs / rz0)
};
// Energy-norm stopping rule of the forcing schedule.  PCG from x_0 = 0 gains inc_j = alpha_j (r_j . z_j) of |x|_A^2 per iteration, and the squared
// energy error after k iterations is the sum of all LATER gains (Hestenes & Stiefel 1952; Strakos & Tichy 2002).  The later gains are extrapolated
// geometrically from the last four: q = (inc_{k-1} + inc_{k-2}) / (inc_{k-3} + inc_{k-4}) is the decay per two iterations, the remainder
// (inc_{k-1} + inc_{k-2}) q / (1 - q).  Unlike a residual norm this bounds what an LM step is about -- the share of the model decrease still
// missing -- whatever the conditioning and the preconditioner.  `k` = iterations done (>= 4), ring = einc.
__device__ __forceinline__ bool cg_energy_stop(const double* ring, double esum, double etol2, int k) {
  if (!(etol2 > 0.0) || k < 4) return false;
  const double a = ring[(k - 1) & 3] + ring[(k - 2) & 3], b = ring[(k - 3) & 3] + ring[(k - 4) & 3];
  if (!(a < b) || !(a >= 0.0)) return false;   // no decay (or a breakdown): carry on
  const double q = a / b;
  // (Round 5 tried a conditioning correction here -- the estimate held against etol2 / kappa, kappa from the current rate q^(1/4) -- for the
  // ill-conditioned far-start problems the round-4 fuzz lost.  Those are caught by the contraction gate of lm_solve instead; with it in place
  // the correction changed no outcome in 420 fuzz trials and cost the spanning-tree start 35 % more iterations: removed.)
  return a * q <= etol2 * esum * (1.0 - q);
}
struct CgArgs {
  uint32_t n;        // cameras
  int nb;            // blocks of the camera kernels (= number of partials)
  int par;           // iteration parity
  double tol, etol2; // (read by the init kernels only: the run's tolerances live in CgScalars)
  int max_iters;
  int stall_limit;   // 0 = off
  const double* Minv;
  const double* b;
  double *xcg, *r, *z, *p, *Ap;
  double* part_a;    // [nb]
  double* part_b;    // [nb]
  const double* zbound; double abs_floor2;   // k_cam_bound's B (device scalar; null or 0: no floor) and floor^2
  CgScalars* sc;
  const double2* q;  // Laplacian form: camera quaternions and
  double* u;         //   u_k = R_k^T p_k, written wherever p is (null otherwise)
  // two-level preconditioner (see k_coarse_*): z = Minv r + P xc, with xc the coarse correction of this iteration; 0 aggregates = off
  uint32_t coarse_n, coarse_chunk;
  const double* xc;  // [3 coarse_n + 1]: correction per aggregate (body frame), then rc . xc
  const double* active;  // 1 / 0 per camera: cameras without an edge take no part in the coarse space either (they must not move)
  double* rc_part;       // [nb][2][3]: this kernel block's share of P^T r for the (at most two) aggregates its 256 cameras belong to; null = the
                         // restriction runs as its own kernel (aggregates narrower than a block)
};
// (P xc)_k = R_k xc[aggregate of k]
__device__ __forceinline__ void coarse_prolong(const CgArgs& a, uint32_t k, double* out) {
  if (a.active[k] == 0.0) { out[0] = out[1] = out[2] = 0.0; return; }
  const uint32_t I = min(k / a.coarse_chunk, a.coarse_n - 1);
  const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
  double R[9];
  qmat(qq, R);
  const double x0 = a.xc[3 * I], x1 = a.xc[3 * I + 1], x2 = a.xc[3 * I + 2];
  out[0] = R[0] * x0 + R[1] * x1 + R[2] * x2; out[1] = R[3] * x0 + R[4] * x1 + R[5] * x2; out[2] = R[6] * x0 + R[7] * x1 + R[8] * x2;
}

// x = 0, r = b, z = Minv r, p = z, partial r.z
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_init(CgArgs a) {
  __shared__ double lds[8];
  double v = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    const double r[3] = {a.b[k3], a.b[k3 + 1], a.b[k3 + 2]};
    double z[3];
    sym3_mulvec(a.Minv + 6 * (size_t)k, r, z);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.xcg[k3 + c] = 0.0; a.r[k3 + c] = r[c]; a.z[k3 + c] = z[c]; a.p[k3 + c] = z[c]; v += r[c] * z[c]; }
    if (a.u) {
      const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
      double uu[3];
      rot_transpose_apply(qq, z, uu);
      a.u[k3] = uu[0]; a.u[k3 + 1] = uu[1]; a.u[k3 + 2] = uu[2];
    }
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_b[blockIdx.x] = t;
}
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_init_fin(CgArgs a) {
  __shared__ double lds[8];
  const double rz = sum_partials_bcast(a.part_b, a.nb, lds);
  if (threadIdx.x == 0) {
    const double bound = a.zbound ? *a.zbound : 0.0, rz_abs = bound > 0.0 ? a.abs_floor2 / bound : 0.0;
    a.sc->rz_abs = rz_abs;
    a.sc->rz[0] = rz; a.sc->rz[1] = rz; a.sc->rz0 = rz; a.sc->best_rel = 1.0;
    a.sc->done = !(rz > rz_abs); a.sc->last_rel = a.sc->done ? 0.0 : 1.0;   // (nothing to solve: converged, not "stopped above the tolerance")
    a.sc->iters = 0; a.sc->stall = 0; a.sc->stalled = 0; a.sc->done_seen = a.sc->done; a.sc->tol = cg_tol_with_floor(a.tol, rz_abs, rz);
    a.sc->etol2 = a.etol2; a.sc->esum = 0.0; a.sc->einc[0] = a.sc->einc[1] = a.sc->einc[2] = a.sc->einc[3] = 0.0;
  }
}
// Continue a stopped solve to a tighter tolerance: the vectors, rz and the iteration count are exactly what the stopping iteration left
// (see done_seen), so the iterates that follow are those of a solve that ran at `tol` from the start.
__global__ void k_cg_resume(CgScalars* sc, double tol, double etol2, int max_iters) {
  tol = cg_tol_with_floor(tol, sc->rz_abs, sc->rz0);
  sc->tol = tol; sc->etol2 = etol2;
  sc->done = !(sc->rz0 > 0.0) || !(sc->last_rel > tol) || sc->iters >= max_iters || sc->stalled;
  sc->done_seen = sc->done;
}
// partial p.Ap
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_dot(CgArgs a) {
  if (a.sc->done) return;
  __shared__ double lds[8];
  double v = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    v = a.p[k3] * a.Ap[k3] + a.p[k3 + 1] * a.Ap[k3 + 1] + a.p[k3 + 2] * a.Ap[k3 + 2];
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_a[blockIdx.x] = t;
}
// alpha = rz / pAp; x += alpha p; r -= alpha Ap; z = Minv r; partial r.z
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_update(CgArgs a) {
  const int done = a.sc->done;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.sc->done_seen = done;   // (nobody writes `done` during this launch)
  if (done) return;
  __shared__ double lds[8];
  const double pAp = sum_partials_bcast(a.part_a, a.nb, lds);
  const double alpha = a.sc->rz[a.par] / pAp;
  if (blockIdx.x == 0 && threadIdx.x == 0) { const double inc = alpha * a.sc->rz[a.par]; a.sc->einc[a.sc->iters & 3] = inc; a.sc->esum += inc; }
  double v = 0.0, rc6[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    double r[3], z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.xcg[k3 + c] += alpha * a.p[k3 + c]; r[c] = a.r[k3 + c] - alpha * a.Ap[k3 + c]; a.r[k3 + c] = r[c]; }
    sym3_mulvec(a.Minv + 6 * (size_t)k, r, z);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.z[k3 + c] = z[c]; v += r[c] * z[c]; }
    if (a.rc_part && a.active[k] != 0.0) {   // two-level preconditioner: this camera's term of P^T r, for the first or the second aggregate of the block
      const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
      double uu[3];
      rot_transpose_apply(qq, r, uu);
      const uint32_t I = min(k / a.coarse_chunk, a.coarse_n - 1), I0 = min((blockIdx.x * GSFM_BLOCK) / a.coarse_chunk, a.coarse_n - 1);
      const int sel = I != I0;
#pragma unroll
      for (int c = 0; c < 3; ++c) { rc6[c] = sel ? 0.0 : uu[c]; rc6[3 + c] = sel ? uu[c] : 0.0; }
    }
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_b[blockIdx.x] = t;
  if (a.rc_part) {
    __shared__ double l6[GSFM_BLOCK / 64][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { const double w = wave_sum(rc6[c]); if ((threadIdx.x & 63) == 0) l6[threadIdx.x >> 6][c] = w; }
    __syncthreads();
    if (threadIdx.x < 6) {
      double sum = 0.0;
      for (int w = 0; w < GSFM_BLOCK / 64; ++w) sum += l6[w][threadIdx.x];
      a.rc_part[6 * (size_t)blockIdx.x + threadIdx.x] = sum;
    }
  }
}
// beta = rz_new / rz; p = z + beta p; convergence test
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_pupdate(CgArgs a) {
  if (a.sc->done_seen) return;   // not `done`: block 0 of THIS launch sets it, and every block must still finish the p update (resumable state)
  __shared__ double lds[8];
  double rz_new = sum_partials_bcast(a.part_b, a.nb, lds);
  if (a.coarse_n) rz_new += a.xc[3 * a.coarse_n];   // r . (Minv r + P xc) = r . Minv r + (P^T r) . xc
  const double rz_old = a.sc->rz[a.par];
  const double beta = rz_new / rz_old;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    double pn[3], zc[3] = {0.0, 0.0, 0.0};
    if (a.coarse_n) coarse_prolong(a, k, zc);
#pragma unroll
    for (int c = 0; c < 3; ++c) { pn[c] = (a.z[k3 + c] + zc[c]) + beta * a.p[k3 + c]; a.p[k3 + c] = pn[c]; }
    if (a.u) {
      const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
      double uu[3];
      rot_transpose_apply(qq, pn, uu);
      a.u[k3] = uu[0]; a.u[k3 + 1] = uu[1]; a.u[k3 + 2] = uu[2];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.sc->rz[a.par ^ 1] = rz_new;
    const int it = a.sc->iters + 1;
    a.sc->iters = it;
    const double rel = sqrt(rz_new / a.sc->rz0);
    a.sc->last_rel = rel;
    // Every block of this launch finishes its p update (the entry test reads done_seen); every later kernel observes the flag at its entry.
    if (!(rel > a.sc->tol) || it >= a.max_iters || cg_energy_stop(a.sc->einc, a.sc->esum, a.sc->etol2, it)) a.sc->done = 1;
    if (a.stall_limit > 0) {  // numerically singular system: the residual plateaus at rounding level
      if (rel < 0.5 * a.sc->best_rel) { a.sc->best_rel = rel; a.sc->stall = 0; }
      else if (++a.sc->stall >= a.stall_limit) { a.sc->done = 1; a.sc->stalled = 1; }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Two-level preconditioner for spatially coherent graphs (block-Jacobi alone needs hundreds of PCG iterations per step there: the
// condition number grows with the square of the graph's diameter).  In the body frame u_k = R_k^T eta_k the normal matrix of the
// Laplacian form is a graph Laplacian with one symmetric 3 x 3 weight per edge, whose near-null vectors are the constants (the global
// gauge rotation), so the coarse space is one 3-vector per aggregate = contiguous chunk of the locality ordering, rotated by R_k:
//   z = Minv r + P Ac^-1 P^T r,   (P v)_k = R_k v[agg(k)],   Ac = P^T A P  (3 n_agg square, assembled per LM step, inverted on the host).
// Additive, symmetric positive definite: PCG's answer does not depend on it, only its iteration count does.
// ------------------------------------------------------------------------------------------
struct CoarseArgs {
  uint32_t n, n_agg, chunk;     // cameras, aggregates, cameras per aggregate
  const double2* q;
  const double* r;              // residual, 3 per camera
  double* rc;                   // [3 n_agg]  P^T r
  const double* Ainv;           // [nc x nc], symmetric
  double* xc;                   // [nc + 1]   Ainv rc, then rc . xc
  const int* done;
  const double* active;
  const double* rc_part;        // non-null: rc is the fixed-order sum of the camera blocks' shares written by k_cg_update ([nb][2][3])
  uint32_t nb;
};
__global__ void __launch_bounds__(GSFM_BLOCK) k_coarse_restrict(CoarseArgs a) {
  if (a.done && *a.done) return;
  __shared__ double lds[8];
  const uint32_t I = blockIdx.x, lo = I * a.chunk, hi = (I + 1 == a.n_agg) ? a.n : min(a.n, lo + a.chunk);
  double acc[3] = {0.0, 0.0, 0.0};
  for (uint32_t k = lo + threadIdx.x; k < hi; k += GSFM_BLOCK) {
    if (a.active[k] == 0.0) continue;
    const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
    double uu[3];
    rot_transpose_apply(qq, a.r + 3 * (size_t)k, uu);
    acc[0] += uu[0]; acc[1] += uu[1]; acc[2] += uu[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = block_sum_bcast(acc[c], lds);
    if (threadIdx.x == 0) a.rc[3 * I + c] = t;
  }
}
// xc = Ainv rc and rc . xc: one workgroup of 1024 lanes; lane (row, g) sums the columns g, g + groups, ... of its row (Ainv is symmetric, so
// column `row` is read as a row: coalesced over the lanes), the groups are combined through LDS.  3 n_agg <= 384.
#define GSFM_COARSE_MAX_NC 384
__global__ void __launch_bounds__(1024) k_coarse_apply(CoarseArgs a) {
  if (a.done && *a.done) return;
  __shared__ double rcs[GSFM_COARSE_MAX_NC];
  __shared__ double part[1024];
  __shared__ double lds[20];
  const uint32_t nc = 3 * a.n_agg, tid = threadIdx.x, groups = 1024 / nc, row = tid % nc, g = tid / nc;
  for (uint32_t c = tid; c < nc; c += 1024) {
    if (a.rc_part) {   // aggregate I = cameras [I chunk, (I + 1) chunk): the blocks of 256 cameras that overlap it, in order
      const uint32_t I = c / 3, comp = c % 3, lo = I * a.chunk, hi = (I + 1 == a.n_agg) ? a.n : min(a.n, lo + a.chunk);
      double sum = 0.0;
      if (hi > lo) {
        for (uint32_t w = lo / GSFM_BLOCK; w <= (hi - 1) / GSFM_BLOCK && w < a.nb; ++w) {
          const uint32_t I0 = min((w * GSFM_BLOCK) / a.chunk, a.n_agg - 1);
          if (I == I0) sum += a.rc_part[6 * (size_t)w + comp];
          else if (I == I0 + 1) sum += a.rc_part[6 * (size_t)w + 3 + comp];
        }
      }
      rcs[c] = sum;
    } else rcs[c] = a.rc[c];
  }
  __syncthreads();
  double sum = 0.0;
  if (g < groups) {
#pragma unroll 8
    for (uint32_t c = g; c < nc; c += groups) sum += a.Ainv[(size_t)c * nc + row] * rcs[c];
  }
  part[tid] = sum;
  __syncthreads();
  double dot = 0.0;
  if (tid < nc) {
    double x = 0.0;
    for (uint32_t gg = 0; gg < groups; ++gg) x += part[gg * nc + tid];
    a.xc[tid] = x;
    dot = x * rcs[tid];
  }
  // block sum over 1024 lanes
  dot = wave_sum(dot);
  if ((tid & 63) == 0) lds[tid >> 6] = dot;
  __syncthreads();
  if (tid == 0) { double t = 0.0; for (int w = 0; w < 16; ++w) t += lds[w]; a.xc[nc] = t; }
}
// after k_cg_init / k_cg_init_fin: p = z + P xc (and u = R^T p), r.z += rc . xc
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg_init_coarse(CgArgs a) {
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    double zc[3], pn[3];
    coarse_prolong(a, k, zc);
#pragma unroll
    for (int c = 0; c < 3; ++c) { pn[c] = a.z[k3 + c] + zc[c]; a.p[k3 + c] = pn[c]; }
    if (a.u) {
      const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
      double uu[3];
      rot_transpose_apply(qq, pn, uu);
      a.u[k3] = uu[0]; a.u[k3 + 1] = uu[1]; a.u[k3 + 2] = uu[2];
    }
  }
}
__global__ void k_cg_init_coarse_fin(CgArgs a) {
  const double rz = a.sc->rz[0] + a.xc[3 * a.coarse_n];
  a.sc->rz[0] = rz; a.sc->rz[1] = rz; a.sc->rz0 = rz; a.sc->done = !(rz > a.sc->rz_abs); a.sc->done_seen = a.sc->done; a.sc->last_rel = a.sc->done ? 0.0 : 1.0;
  a.sc->tol = cg_tol_with_floor(a.tol, a.sc->rz_abs, rz);
}
// Ac = P^T A P from the stored blocks of the Laplacian form: off-diagonal entry (k -> m) contributes -R_k^T G_k R_k to block (agg k, agg m),
// the diagonal block R_k^T M_k R_k to (agg k, agg k).  G lanes per row; a lane sums its consecutive entries that fall into the same
// aggregate before touching memory (rows are sorted by neighbour, so that is most of them), then adds with 64-bit integer atomics on a
// fixed-point image of the matrix (coarse_flush): bit-identical from run to run.  Ac is zero-filled before the launch.
struct CoarseAsmArgs {
  uint32_t n_rows, row_base, G, n_agg, chunk;   // owned rows; global camera index of row 0
  const uint32_t* row_ptr;
  const uint32_t* col;
  const double2 *h0, *h1, *h2;
  const double* Mblk;
  const double2* q;
  double* Ac;          // fixed point while being summed (coarse_flush), doubles after k_coarse_unscale
  const double* scale;
};
// Sums in 64-bit FIXED POINT: integer addition is associative, so the atomics may land in any order and Ac is still the same bits on every
// run (floating-point atomics would make the preconditioner, and through it the PCG path, reproducible to rounding only).  `scale` = 2^e with
// e chosen by k_coarse_scale so that the largest single contribution is below 2^40: 2^22 of them fit before an int64 overflows (an aggregate
// sums <= chunk x degree ~ 2^19), and the resolution of 2^-40 of the largest diagonal entry is far finer than a preconditioner needs.
__device__ __forceinline__ void coarse_flush(double* Ac, uint32_t nc, uint32_t I, uint32_t J, const double* S /* sym 6: 00 01 02 11 12 22 */, double scale) {
  unsigned long long* o = (unsigned long long*)(Ac + (size_t)(3 * I) * nc + 3 * J);
  long long q[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) q[c] = __double2ll_rn(S[c] * scale);
  atomicAdd(o, (unsigned long long)q[0]); atomicAdd(o + 1, (unsigned long long)q[1]); atomicAdd(o + 2, (unsigned long long)q[2]);
  atomicAdd(o + nc, (unsigned long long)q[1]); atomicAdd(o + nc + 1, (unsigned long long)q[3]); atomicAdd(o + nc + 2, (unsigned long long)q[4]);
  atomicAdd(o + 2 * nc, (unsigned long long)q[2]); atomicAdd(o + 2 * nc + 1, (unsigned long long)q[4]); atomicAdd(o + 2 * nc + 2, (unsigned long long)q[5]);
}
// scale[0] = 2^e, scale[1] = 2^-e from the largest diagonal entry of the damped diagonal blocks (every |G_ab| of an edge is below it: G is
// positive semi-definite and M_k sums the G of camera k's edges)
__global__ void __launch_bounds__(GSFM_BLOCK) k_coarse_scale(const double* __restrict__ Mblk, uint32_t n_rows, uint32_t row_base, double* partials, double* scale, int pass) {
  __shared__ double lds[8];
  double v = 0.0;
  if (pass == 0) {
    const uint32_t r = blockIdx.x * GSFM_BLOCK + threadIdx.x;
    if (r < n_rows) { const double* M = Mblk + 6 * (size_t)(row_base + r); v = fmax(fabs(M[0]), fmax(fabs(M[3]), fabs(M[5]))); }
    v = block_max_bcast(v, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = v;
  } else {   // one block: partials -> the power of two
    for (uint32_t k = threadIdx.x; k < n_rows /* = number of partials */; k += GSFM_BLOCK) v = fmax(v, partials[k]);
    v = block_max_bcast(v, lds);
    if (threadIdx.x == 0) {
      int e = 0;
      if (v > 0.0 && isfinite(v)) { (void)frexp(v, &e); e = 40 - e; }   // v < 2^(40 - e')... v * 2^e < 2^40
      scale[0] = ldexp(1.0, e); scale[1] = ldexp(1.0, -e);
    }
  }
}
// fixed point -> double, in place
__global__ void __launch_bounds__(GSFM_BLOCK) k_coarse_unscale(double* Ac, size_t n, const double* scale) {
  const size_t t = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (t < n) { const long long q = ((const long long*)Ac)[t]; Ac[t] = (double)q * scale[1]; }
}
// S = R^T Sym R for a symmetric 3 x 3 given as (00 01 02 11 12 22)
__device__ __forceinline__ void sym3_congruence_T(const double* R, const double* M, double* S) {
  const double m[9] = {M[0], M[1], M[2], M[1], M[3], M[4], M[2], M[4], M[5]};
  double t[9];   // t = M R
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) t[3 * r + c] = m[3 * r] * R[c] + m[3 * r + 1] * R[3 + c] + m[3 * r + 2] * R[6 + c];
  // S = R^T t
  S[0] = R[0] * t[0] + R[3] * t[3] + R[6] * t[6]; S[1] = R[0] * t[1] + R[3] * t[4] + R[6] * t[7]; S[2] = R[0] * t[2] + R[3] * t[5] + R[6] * t[8];
  S[3] = R[1] * t[1] + R[4] * t[4] + R[7] * t[7]; S[4] = R[1] * t[2] + R[4] * t[5] + R[7] * t[8]; S[5] = R[2] * t[2] + R[5] * t[5] + R[8] * t[8];
}
__global__ void __launch_bounds__(GSFM_BLOCK) k_coarse_assemble(CoarseAsmArgs a) {
  const uint32_t t = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const uint32_t row = t / a.G, lane = t % a.G;
  const bool valid = row < a.n_rows;
  const double scale = a.scale[0];
  const uint32_t cam = a.row_base + (valid ? row : a.n_rows - 1);
  const uint32_t nc = 3 * a.n_agg, I = min(cam / a.chunk, a.n_agg - 1);
  // blocks (I, I-1), (I, I), (I, I+1): in a coherent graph nearly every entry; summed over the wavefront below, one set of atomics each
  double near[3][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
  if (valid) {
    double R[9];
    qmat(load_q(a.q, cam), R);
    uint32_t curJ = 0xffffffffu;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t end = a.row_ptr[row + 1];
    for (uint32_t d = a.row_ptr[row] + lane; d < end; d += a.G) {
      const uint32_t m = a.col[d] & 0x7fffffffu, J = min(m / a.chunk, a.n_agg - 1);
      const double2 A = a.h0[d], B = a.h1[d], C = a.h2[d];
      const double Gs[6] = {A.x, A.y, B.x, B.y, C.x, C.y};
      double S[6];
      sym3_congruence_T(R, Gs, S);
      const uint32_t rel = J + 1 - I;   // 0, 1, 2 for the three near blocks (unsigned wrap-around puts everything else above 2)
      if (rel <= 2) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
          if (rel == (uint32_t)w) {
#pragma unroll
            for (int c = 0; c < 6; ++c) near[w][c] -= S[c];
          }
        continue;
      }
      if (J != curJ) {
        if (curJ != 0xffffffffu) coarse_flush(a.Ac, nc, I, curJ, acc, scale);
        curJ = J;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = 0.0;
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] -= S[c];
    }
    if (curJ != 0xffffffffu) coarse_flush(a.Ac, nc, I, curJ, acc, scale);
    if (lane == 0 && end > a.row_ptr[row]) {   // (a camera without edges is not part of the coarse space)
      double S[6];
      sym3_congruence_T(R, a.Mblk + 6 * (size_t)cam, S);
#pragma unroll
      for (int c = 0; c < 6; ++c) near[1][c] += S[c];
    }
  }
  // one set of atomics per wavefront and block when all its rows belong to the same aggregate (they do, except at the chunk boundaries)
  const uint32_t I0 = __shfl(I, 0);
  const bool uniform = __all(I == I0);
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const uint32_t J = I + (uint32_t)w - 1u;
    if (J >= a.n_agg) continue;          // (I - 1 of the first aggregate wraps around; I + 1 of the last does not exist)
    if (uniform) {
      double sum6[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) sum6[c] = wave_sum(near[w][c]);
      if ((threadIdx.x & 63) == 0) coarse_flush(a.Ac, nc, I0, J, sum6, scale);
    } else if (valid) {
      coarse_flush(a.Ac, nc, I, J, near[w], scale);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Single-reduction PCG (Chronopoulos & Gear): one mat-vec kernel + one vector kernel per iteration.
//   u = M^-1 r, w = A u, gamma = r.u, delta = w.u
//   beta = gamma/gamma_prev, alpha = gamma / (delta - beta gamma / alpha_prev)
//   p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s, u = M^-1 r
// gamma partials are produced by the vector kernel (for the NEXT iteration), delta partials by the
// mat-vec; every block re-sums the partials in the same order, so all blocks (and all ranks) see
// bit-identical scalars and no finalize launch or atomics are needed.
// ------------------------------------------------------------------------------------------
#define GSFM_MV_MAX_PARTIALS 8192   // the fused mat-vec runs `reps` row groups per workgroup so that its delta partials stay below this
// The PCG's status for the host WITHOUT a stream synchronisation: the last node of a chunk copies the scalar block into mapped host memory and
// stamps it with a device-resident count of such posts (system-scope release); the host polls the stamp.  A read-back costs a blit kernel, the
// return of hipStreamSynchronize and the next launch's way to the GPU -- 14 + 4 + 25 us of idle GPU per look in the latency regime (10k
// cameras / 200k edges: 16 looks per solve, a quarter of the PCG time).  No per-call kernel argument: the node is part of the captured chunk.
#define GSFM_MAIL_WORDS 32
__global__ void k_pcg_mail(const double* __restrict__ sc, int nwords, double* mail, double* counter) {
  for (int k = 0; k < nwords; ++k) mail[k] = sc[k];
  const double c = *counter + 1.0;
  *counter = c;
  __threadfence_system();
  __hip_atomic_store(mail + GSFM_MAIL_WORDS, c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The LM loop's look at a trial point in ONE launch: the step's five sums and the trial cost's (the reductions k_sum_partials_multi /
// k_sum_partials would have launched: same routine, same order, same bits, written to the same scalars), then the scalar block's post.
__global__ void __launch_bounds__(GSFM_BLOCK) k_trial_post(double* scal, int sc_step, int sc_trial, const double* __restrict__ step_part, int nb_cam,
                                                           const double* __restrict__ cost_part, int nb_cost, int nwords, double* mail, double* counter, int sc_z) {
  __shared__ double lds[8];
  for (int c = 0; c < 5; ++c) {
    const double t = sum_partials_bcast(step_part + (size_t)c * nb_cam, nb_cam, lds);
    if (threadIdx.x == 0) scal[sc_step + c] = t;
  }
  if (sc_z >= 0) {   // (k_cam_step's sixth sum: the per-camera Jacobi estimate of a loose step's error)
    const double t = sum_partials_bcast(step_part + (size_t)5 * nb_cam, nb_cam, lds);
    if (threadIdx.x == 0) scal[sc_z] = t;
  }
  const double t = sum_partials_bcast(cost_part, nb_cost, lds);
  if (threadIdx.x != 0) return;
  scal[sc_trial] = t;
  for (int k = 0; k < nwords; ++k) mail[k] = scal[k];
  const double c = *counter + 1.0;
  *counter = c;
  __threadfence_system();
  __hip_atomic_store(mail + GSFM_MAIL_WORDS, c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Cg2Scalars {
  double gamma[2];   // parity-indexed gamma_i
  double alpha[2];
  double gamma0;
  double last_rel;
  int done;
  int iters;
  double tol;        // relative tolerance of the current run (device-resident: see CgScalars::tol)
  double etol2, esum, einc[4];   // energy-norm stopping rule of the loose solves (cg_energy_stop): inc_j = alpha_j gamma_j
  double rz_abs;     // absolute floor on gamma = r.z (k_cam_bound): `tol` never drops below sqrt(rz_abs / gamma0)
};
struct Cg2Args {
  uint32_t n;            // cameras
  int nb_cam;            // blocks of the camera kernels
  int n_part_d;          // number of delta partials (mat-vec blocks, or nb_cam when sharded)
  int par;               // iteration parity
  int first;             // 1 on iteration 0
  int max_iters;
  double tol, etol2;     // (read by k_cg2_init only: the run's tolerances live in Cg2Scalars)
  const double* zbound; double abs_floor2;   // k_cam_bound's B (device scalar; null or 0: no floor) and floor^2
  const double* Minv;
  const double* b;
  double *x, *r, *u, *w, *p, *s;
  double* part_g;        // [2][nb_cam]  (parity-indexed)
  double* part_d;        // [n_part_d]
  Cg2Scalars* sc;
  const double2* q;      // Laplacian form: camera quaternions and
  double* urot;          //   urot_k = R_k^T u_k, written wherever u is (null otherwise): the vector the mat-vec gathers
  // Sharded problems: w lives in the all-gather buffer, one slot of `w_stride` doubles per rank = its slice of w (3 * w_slice doubles)
  // followed by `w_tail` delta partials of its own rows -- the partial dot products travel with A u in the ONE collective of the
  // iteration, every rank sums all tails in the same order.  w_stride == 0: w is a plain vector and part_d a plain array.
  uint32_t w_stride, w_slice, w_tail;
};
__device__ __forceinline__ size_t cg2_w_index(const Cg2Args& a, uint32_t k) {
  return a.w_stride ? (size_t)(k / a.w_slice) * a.w_stride + 3 * (size_t)(k % a.w_slice) : 3 * (size_t)k;
}

// x = 0, r = b, u = M^-1 r, p = s = 0, gamma_0 partials
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg2_init(Cg2Args a) {
  __shared__ double lds[8];
  double v = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    const double r[3] = {a.b[k3], a.b[k3 + 1], a.b[k3 + 2]};
    double u[3];
    sym3_mulvec(a.Minv + 6 * (size_t)k, r, u);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.x[k3 + c] = 0.0; a.r[k3 + c] = r[c]; a.u[k3 + c] = u[c]; a.p[k3 + c] = 0.0; a.s[k3 + c] = 0.0; v += r[c] * u[c]; }
    if (a.urot) {
      const Quat qq{a.q[2 * (size_t)k].x, a.q[2 * (size_t)k].y, a.q[2 * (size_t)k + 1].x, a.q[2 * (size_t)k + 1].y};
      double uu[3];
      rot_transpose_apply(qq, u, uu);
      a.urot[k3] = uu[0]; a.urot[k3 + 1] = uu[1]; a.urot[k3 + 2] = uu[2];
    }
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_g[blockIdx.x] = t;
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.sc->done = 0; a.sc->iters = 0; a.sc->last_rel = 1.0; a.sc->gamma0 = 0.0; a.sc->tol = a.tol;
    { const double bound = a.zbound ? *a.zbound : 0.0; a.sc->rz_abs = bound > 0.0 ? a.abs_floor2 / bound : 0.0; }
    a.sc->etol2 = a.etol2; a.sc->esum = 0.0; a.sc->einc[0] = a.sc->einc[1] = a.sc->einc[2] = a.sc->einc[3] = 0.0; }
}
// Continue a stopped solve to a tighter tolerance.  The recurrence stops at a mat-vec ENTRY (every workgroup takes the same decision from
// the same gamma partials, nothing of the iteration has been written), so clearing the flag lets the next mat-vec -- launched with the
// parity and `first` flag of the iteration that stopped -- take the decision again, against the new tolerance.
__global__ void k_cg2_resume(Cg2Scalars* sc, double tol, double etol2) {
  sc->tol = cg_tol_with_floor(tol, sc->rz_abs, sc->gamma0); sc->etol2 = etol2;
  sc->done = 0;
}

// w = A u on the owned rows (G lanes per row, `reps` row groups per workgroup) + delta partials (unsharded only).
// Written for the latency regime: every load that does not depend on another load of this kernel -- the PCG scalars, the gamma
// partials, the row bounds, the first trip's column / blocks and its gathered vector entry -- is requested before the first use of
// any of them, so a workgroup pays ~3 dependent memory round trips (row bounds -> column -> gather) instead of one per stage.
struct MatvecCgArgs { MatvecArgs mv; Cg2Args cg; int with_dots; uint32_t reps; };
template <bool LAP>
__device__ __forceinline__ void mv_entry(const MatvecArgs& a, const double* Rk, uint32_t m, const double2& A, const double2& B, const double2& C,
                                         const double2& D, double E, const double* v, double& y0, double& y1, double& y2) {
  if (LAP) {
    const double w0 = Rk[0] * v[0] + Rk[1] * v[1] + Rk[2] * v[2], w1 = Rk[3] * v[0] + Rk[4] * v[1] + Rk[5] * v[2], w2 = Rk[6] * v[0] + Rk[7] * v[1] + Rk[8] * v[2];
    y0 += A.x * w0 + A.y * w1 + B.x * w2;
    y1 += A.y * w0 + B.y * w1 + C.x * w2;
    y2 += B.x * w0 + C.x * w1 + C.y * w2;
  } else {
    y0 += A.x * v[0] + A.y * v[1] + B.x * v[2];
    y1 += B.y * v[0] + C.x * v[1] + C.y * v[2];
    y2 += D.x * v[0] + D.y * v[1] + E * v[2];
  }
}
template <bool LAP>
__global__ void __launch_bounds__(GSFM_BLOCK) k_matvec_cg(MatvecCgArgs aa) {
  __shared__ double lds[8];
  const MatvecArgs& a = aa.mv;
  const Cg2Args& c = aa.cg;
  const double* __restrict__ vec = LAP ? a.u : a.p;   // the gathered vector: R^T u (Laplacian form) or u itself
  // ---- request phase ----
  const int done = c.sc->done, iters = c.sc->iters;
  const double gamma0 = c.sc->gamma0, tol = c.sc->tol;
  const bool estop = cg_energy_stop(c.sc->einc, c.sc->esum, c.sc->etol2, iters);
  double gpart = 0.0;
  for (int k = threadIdx.x; k < c.nb_cam; k += GSFM_BLOCK) gpart += c.part_g[(size_t)c.par * c.nb_cam + k];
  const uint32_t G = a.G, rows_per_group = GSFM_BLOCK / G;
  const uint32_t lane = threadIdx.x % G, sub = threadIdx.x / G;
  uint32_t row = blockIdx.x * aa.reps * rows_per_group + sub;
  bool live = row < a.n_rows;
  uint32_t d = 0, end = 0;
  if (live) { d = a.row_ptr[row] + lane; end = a.row_ptr[row + 1]; }
  bool has = live && d < end;
  uint32_t m = 0;
  double2 A = make_double2(0, 0), B = A, C = A, D = A;
  double E = 0.0, v[3] = {0, 0, 0};
  Quat qk{0, 0, 0, 1};
  if (live && LAP) qk = load_q(a.q, a.row_base + row);
  double M0[6] = {0, 0, 0, 0, 0, 0}, pk0[3] = {0, 0, 0};   // the row owner's diagonal block and vector entry (first row group)
  if (live && lane == 0) {
    const size_t k = a.row_base + row;
#pragma unroll
    for (int t = 0; t < 6; ++t) M0[t] = a.Mblk[6 * k + t];
#pragma unroll
    for (int t = 0; t < 3; ++t) pk0[t] = a.p[3 * k + t];
  }
  if (has) {
    m = __builtin_nontemporal_load(a.col + d) & 0x7fffffffu;
    A = nt_load2(a.h0 + d); B = nt_load2(a.h1 + d); C = nt_load2(a.h2 + d);
    if (!LAP) { D = nt_load2(a.h3 + d); E = __builtin_nontemporal_load(a.h4 + d); }
    const double* vm = vec + 3 * (size_t)m;
    v[0] = vm[0]; v[1] = vm[1]; v[2] = vm[2];
  }
  // ---- convergence (same decision in every workgroup: same partials, same order) ----
  const double gamma = block_sum_bcast(gpart, lds);
  if (done) return;
  bool conv;
  if (c.first) {
    const double rz_abs = c.sc->rz_abs;   // (written by k_cg2_init, the launch before)
    conv = !(gamma > rz_abs);
    if (blockIdx.x == 0 && threadIdx.x == 0) { c.sc->gamma0 = gamma; c.sc->tol = cg_tol_with_floor(tol, rz_abs, gamma); if (conv) { c.sc->done = 1; c.sc->last_rel = 0.0; } }
  } else {
    const double rel = sqrt(gamma / gamma0);
    // the iteration cap is applied here, at a kernel entry, from a counter written by the PREVIOUS launch: every workgroup takes
    // the same decision, and no workgroup of a vector-update launch can see the flag flip half way through an update of x
    conv = !(rel > tol) || iters >= c.max_iters || estop;
    if (blockIdx.x == 0 && threadIdx.x == 0) { c.sc->last_rel = rel; if (conv) c.sc->done = 1; }
  }
  if (conv) return;
  // ---- rows ----
  double dpart = 0.0;
  for (uint32_t rep = 0; rep < aa.reps; ++rep) {
    if (rep > 0) {
      row = (blockIdx.x * aa.reps + rep) * rows_per_group + sub;
      live = row < a.n_rows;
      d = 0; end = 0;
      if (live) { d = a.row_ptr[row] + lane; end = a.row_ptr[row + 1]; if (LAP) qk = load_q(a.q, a.row_base + row); }
      has = false;   // no prefetched entry: the loop below starts at d
    }
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (live) {
      double Rk[9];
      if (LAP) qmat(qk, Rk);
      if (has) { mv_entry<LAP>(a, Rk, m, A, B, C, D, E, v, y0, y1, y2); d += G; }
      for (; d < end; d += G) {
        const uint32_t mm = __builtin_nontemporal_load(a.col + d) & 0x7fffffffu;
        const double2 A2 = nt_load2(a.h0 + d), B2 = nt_load2(a.h1 + d), C2 = nt_load2(a.h2 + d);
        double2 D2 = make_double2(0, 0); double E2 = 0.0;
        if (!LAP) { D2 = nt_load2(a.h3 + d); E2 = __builtin_nontemporal_load(a.h4 + d); }
        const double* vm = vec + 3 * (size_t)mm;
        const double vv[3] = {vm[0], vm[1], vm[2]};
        mv_entry<LAP>(a, Rk, mm, A2, B2, C2, D2, E2, vv, y0, y1, y2);
      }
    }
    for (uint32_t off = G >> 1; off > 0; off >>= 1) {
      y0 += __shfl_down(y0, off, G); y1 += __shfl_down(y1, off, G); y2 += __shfl_down(y2, off, G);
    }
    if (live && lane == 0) {
      const size_t k = a.row_base + row;
      if (rep > 0) {
#pragma unroll
        for (int t = 0; t < 6; ++t) M0[t] = a.Mblk[6 * k + t];
#pragma unroll
        for (int t = 0; t < 3; ++t) pk0[t] = a.p[3 * k + t];
      }
      double mp[3];
      sym3_mulvec(M0, pk0, mp);
      const double sgn = LAP ? -1.0 : 1.0;
      const double w0 = mp[0] + sgn * y0, w1 = mp[1] + sgn * y1, w2 = mp[2] + sgn * y2;
      a.y[3 * k] = w0; a.y[3 * k + 1] = w1; a.y[3 * k + 2] = w2;
      dpart += w0 * pk0[0] + w1 * pk0[1] + w2 * pk0[2];
    }
  }
  if (aa.with_dots) {
    const double t = block_sum_bcast(dpart, lds);
    if (threadIdx.x == 0) aa.cg.part_d[blockIdx.x] = t;
  }
}

// sharded path: delta partials over ALL cameras after the all-gather of w (identical on every rank)
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg2_dots(Cg2Args a) {
  if (a.sc->done) return;
  __shared__ double lds[8];
  double v = 0.0;
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  if (k < a.n) {
    const size_t k3 = 3 * (size_t)k;
    v = a.w[k3] * a.u[k3] + a.w[k3 + 1] * a.u[k3 + 1] + a.w[k3 + 2] * a.u[k3 + 2];
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_d[blockIdx.x] = t;
}

// alpha, beta and all five vector updates; gamma partials of the next iteration.  Like the mat-vec above, all loads are requested
// before the first reduction (one memory round trip, then two workgroup reductions, then the stores).
__global__ void __launch_bounds__(GSFM_BLOCK) k_cg2_step(Cg2Args a) {
  __shared__ double lds[8];
  const int done = a.sc->done;
  const double gamma_prev = a.sc->gamma[a.par ^ 1], alpha_prev = a.sc->alpha[a.par ^ 1];
  double gpart = 0.0, dsum = 0.0;
  for (int k = threadIdx.x; k < a.nb_cam; k += GSFM_BLOCK) gpart += a.part_g[(size_t)a.par * a.nb_cam + k];
  if (a.w_stride) {
    for (int k = threadIdx.x; k < a.n_part_d; k += GSFM_BLOCK) dsum += a.w[(size_t)(k / a.w_tail) * a.w_stride + 3 * (size_t)a.w_slice + k % a.w_tail];
  } else for (int k = threadIdx.x; k < a.n_part_d; k += GSFM_BLOCK) dsum += a.part_d[k];
  const uint32_t k = blockIdx.x * GSFM_BLOCK + threadIdx.x;
  const bool live = k < a.n;
  const size_t k3 = 3 * (size_t)(live ? k : 0), kw = cg2_w_index(a, live ? k : 0);
  double uo[3], po[3], wo[3], so[3], xo[3], ro[3], Mi[6];
  Quat qq{0, 0, 0, 1};
#pragma unroll
  for (int c = 0; c < 3; ++c) { uo[c] = a.u[k3 + c]; po[c] = a.p[k3 + c]; wo[c] = a.w[kw + c]; so[c] = a.s[k3 + c]; xo[c] = a.x[k3 + c]; ro[c] = a.r[k3 + c]; }
#pragma unroll
  for (int c = 0; c < 6; ++c) Mi[c] = a.Minv[2 * k3 + c];
  if (a.urot) qq = load_q(a.q, live ? k : 0);
  const double gamma = block_sum_bcast(gpart, lds);
  const double delta = block_sum_bcast(dsum, lds);
  if (done) return;
  double beta, alpha;
  if (a.first) { beta = 0.0; alpha = gamma / delta; }
  else {
    beta = gamma / gamma_prev;
    alpha = gamma / (delta - beta * gamma / alpha_prev);
  }
  double v = 0.0;
  if (live) {
    double r[3], u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p = uo[c] + beta * po[c];
      const double s = wo[c] + beta * so[c];
      a.p[k3 + c] = p; a.s[k3 + c] = s;
      a.x[k3 + c] = xo[c] + alpha * p;
      r[c] = ro[c] - alpha * s;
      a.r[k3 + c] = r[c];
    }
    sym3_mulvec(Mi, r, u);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.u[k3 + c] = u[c]; v += r[c] * u[c]; }
    if (a.urot) {
      double uu[3];
      rot_transpose_apply(qq, u, uu);
      a.urot[k3] = uu[0]; a.urot[k3 + 1] = uu[1]; a.urot[k3 + 2] = uu[2];
    }
  }
  const double t = block_sum_bcast(v, lds);
  if (threadIdx.x == 0) a.part_g[(size_t)(a.par ^ 1) * a.nb_cam + blockIdx.x] = t;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int it = a.sc->iters;
    const double inc = alpha * gamma;
    a.sc->gamma[a.par] = gamma; a.sc->alpha[a.par] = alpha; a.sc->einc[it & 3] = inc; a.sc->esum += inc; a.sc->iters = it + 1;
  }
}

}  // namespace gsfm
