// Device kernels of the 1DSfM relative-translation filter (include/gsfm_pos.h, gsfm_pos_filter_relative_translations): Theia's
// FilterViewPairsFromRelativeTranslation under the reproducible definition of that header.
//
// Edge sweeps: world directions (the position problem's routine), their mean and variance (a fixed number of partials in a fixed order),
// the projections when the caller wants them, and the bad-weight sum (one thread per edge, projections in ascending order).
//
// Ordering (k_tf_order), the hot path.  One workgroup owns one projection from the first pass to the last; the projections run side by
// side and no workgroup ever reads what another writes, so nothing waits on anything outside its own barriers.  Per camera the workgroup
// keeps qin, qout (64-bit integer weight sums over arcs from / to live cameras), indeg (live incoming arcs), the pass that removed it
// and one slot of the source work list: 28 B, in LDS when that fits and in global memory otherwise (the same code, TfState).  All
// updates are integer atomics, so the state after a pass does not depend on the order of the lanes.
//   source pass: the cameras on the work list (indeg == 0 at the start of the pass) are removed, one wavefront per camera, lanes over its
//                CSR row; a neighbour whose indeg reaches 0 is appended to the list for the next pass (it is appended once in its life,
//                so one list of n_cams slots serves all passes).
//   score pass:  taken when the list is empty.  The argmax of (qout + 2^32) / (qin + 2^32) over the live cameras, smallest index among
//                equals, through per-group maxima (64 cameras a group) that are recomputed only for groups a removal touched; then the
//                whole workgroup walks the picked camera's row.
// Every pass removes at least one camera, so the loop ends after at most n_cams passes.  The projections are recomputed from the 24-byte
// directions by tf_project, whose every operation is an explicitly rounded one (a product and two fma): the ordering, the bad-weight
// sum and proj_out get the same bits wherever the compiler inlines it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pos_kernels.hpp"

namespace gsfm {

#define GSFM_TF_PARTS 256                 // partials of the mean / variance sums (a constant: the order of the sums is fixed)
#define GSFM_TF_LIVE 0xffffffffu          // pass number of a camera that has not been removed yet
#define GSFM_TF_ABSENT 0xfffffffeu        // ... of a camera without an edge (not a node)
#define GSFM_TF_GROUP 64                  // cameras per group maximum

__device__ __forceinline__ double tf_project(const double* __restrict__ dir_e, size_t e, double a0, double a1, double a2) {
  return fma(dir_e[3 * e + 2], a2, fma(dir_e[3 * e + 1], a1, dir_e[3 * e] * a0));
}
// q = floor(|p| 2^32 + 0.5) (the scaling is exact, so a contraction of the two operations cannot change the result)
__device__ __forceinline__ unsigned long long tf_weight(double p) { return (unsigned long long)floor(fabs(p) * 4294967296.0 + 0.5); }

__global__ void __launch_bounds__(256) k_tf_directions(uint32_t n_edges, const uint32_t* __restrict__ ei, const double* __restrict__ rot_aa,
                                                       const double* __restrict__ rel_t, double* __restrict__ dir_e) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  double d[3];
  pos_world_direction(rot_aa + 3 * (size_t)ei[e], rel_t + 3 * e, d);
  for (int c = 0; c < 3; ++c) dir_e[3 * e + c] = d[c];
}

// part[3 b + c] = sum over the edges of block b's stride of (d_c - center_c)^(square ? 2 : 1); center NULL = 0
__global__ void __launch_bounds__(256) k_tf_moment(const double* __restrict__ dir_e, uint32_t n_edges, const double* __restrict__ center, int square,
                                                   double* __restrict__ part) {
  __shared__ double red[3][256];
  const double c0 = center ? center[0] : 0.0, c1 = center ? center[1] : 0.0, c2 = center ? center[2] : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (size_t)GSFM_TF_PARTS * 256) {
    const double a = dir_e[3 * e] - c0, b = dir_e[3 * e + 1] - c1, c = dir_e[3 * e + 2] - c2;
    if (square) { s0 += a * a; s1 += b * b; s2 += c * c; } else { s0 += a; s1 += b; s2 += c; }
  }
  red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) part[3 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}
// out[c] = (sum of the partials in a fixed tree) / denom   (denom <= 0: 0, the variance of a single edge)
__global__ void __launch_bounds__(256) k_tf_moment_final(const double* __restrict__ part, double denom, double* __restrict__ out) {
  __shared__ double red[3][256];
  for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = threadIdx.x < GSFM_TF_PARTS ? part[3 * threadIdx.x + c] : 0.0;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) out[threadIdx.x] = denom > 0.0 ? red[threadIdx.x][0] / denom : 0.0;
}

// proj_out[e n_axes + k] = d_e . axis_k
__global__ void __launch_bounds__(256) k_tf_proj(uint32_t n_edges, const double* __restrict__ dir_e, const double* __restrict__ axes, int n_axes,
                                                 double* __restrict__ proj_out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  for (int k = 0; k < n_axes; ++k) proj_out[e * (size_t)n_axes + k] = tf_project(dir_e, e, axes[3 * k], axes[3 * k + 1], axes[3 * k + 2]);
}

struct TfOrderArgs {
  uint32_t n_cams, n_groups;
  const uint32_t* row_ptr;   // n_cams + 1
  const uint32_t* nbr;       // 2E: neighbour of each directed entry
  const uint32_t* ent;       // 2E: 2 e + side (side 1: the row is the edge's second camera)
  const double* dir_e;       // E x 3
  const double* axes;        // n_axes x 3
  uint32_t* pass_out;        // n_axes x n_cams: the pass that removed each camera (GSFM_TF_ABSENT: no edge)
  uint32_t* counts;          // n_axes x 2: passes, score picks
  // state of the global-memory path, per projection (unused by the LDS path)
  unsigned long long* g_q;   // n_axes x 2 n_cams
  double* g_gmax;            // n_axes x n_groups
  uint32_t* g_u32;           // n_axes x (2 n_cams + 2 n_groups)   (the pass numbers live in pass_out)
};

struct TfState {
  unsigned long long* qin; unsigned long long* qout;
  double* gmax;
  uint32_t* indeg; uint32_t* pass; uint32_t* list; uint32_t* gidx; uint32_t* dirty;
};
// bytes of dynamic LDS of the LDS path
inline size_t tf_lds_bytes(uint32_t n_cams) {
  const size_t n = n_cams, G = (n + GSFM_TF_GROUP - 1) / GSFM_TF_GROUP;
  return 16 * n + 8 * G + 4 * (3 * n + 2 * G);
}

// (score, index) maximum: the larger score, the smaller index among equal scores
__device__ __forceinline__ void tf_better(double& s, uint32_t& i, double s2, uint32_t i2) {
  if (s2 > s || (s2 == s && i2 < i)) { s = s2; i = i2; }
}
__device__ __forceinline__ void tf_wave_argmax(double& s, uint32_t& i) {
  for (int w = 32; w > 0; w >>= 1) {
    const double s2 = __shfl_xor(s, w);
    const uint32_t i2 = __shfl_xor(i, w);
    tf_better(s, i, s2, i2);
  }
}

// camera u is being removed: its directed entry d's arc leaves the neighbour's sums
__device__ __forceinline__ void tf_remove_entry(const TfOrderArgs& a, const TfState& S, uint32_t d, double a0, double a1, double a2, uint32_t list_base,
                                                uint32_t* n_new) {
  const uint32_t m = a.nbr[d];
  if (S.pass[m] != GSFM_TF_LIVE) return;
  const uint32_t x = a.ent[d], side = x & 1u;
  const double p = tf_project(a.dir_e, x >> 1, a0, a1, a2);
  const unsigned long long q = tf_weight(p);
  const bool out = (p > 0.0) != (side != 0);   // the arc leaves the removed camera
  if (out) {
    atomicAdd(S.qin + m, 0ull - q);
    if (atomicSub(S.indeg + m, 1u) == 1u) S.list[list_base + atomicAdd(n_new, 1u)] = m;   // a new source: removed by the next pass
  } else {
    atomicAdd(S.qout + m, 0ull - q);
  }
  S.dirty[m / GSFM_TF_GROUP] = 1u;
}

template <bool LDS>
__global__ void __launch_bounds__(1024) k_tf_order(TfOrderArgs a) {
  extern __shared__ unsigned long long tf_smem[];
  __shared__ double red_s[16];
  __shared__ uint32_t red_i[16];
  __shared__ uint32_t n_new[3];     // sources appended for pass p + 1 are counted in n_new[(p + 1) % 3]
  __shared__ uint32_t n_present;
  const uint32_t k = blockIdx.x, n = a.n_cams, G = a.n_groups, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, n_waves = nt >> 6;
  TfState S;
  if (LDS) {
    S.qin = tf_smem; S.qout = S.qin + n; S.gmax = (double*)(S.qout + n);
    S.indeg = (uint32_t*)(S.gmax + G); S.pass = S.indeg + n; S.list = S.pass + n; S.gidx = S.list + n; S.dirty = S.gidx + G;
  } else {
    S.qin = a.g_q + (size_t)k * 2 * n; S.qout = S.qin + n; S.gmax = a.g_gmax + (size_t)k * G;
    S.indeg = a.g_u32 + (size_t)k * (2 * (size_t)n + 2 * G); S.list = S.indeg + n; S.gidx = S.list + n; S.dirty = S.gidx + G;
    S.pass = a.pass_out + (size_t)k * n;
  }
  const double a0 = a.axes[3 * k], a1 = a.axes[3 * k + 1], a2 = a.axes[3 * k + 2];
  if (tid < 3) n_new[tid] = 0;
  if (tid == 0) n_present = 0;
  __syncthreads();

  // ---- the sums of every camera over all its arcs; the first sources -------------------------------------------------------------------
  uint32_t mine = 0;
  for (uint32_t v = tid; v < n; v += nt) {
    const uint32_t beg = a.row_ptr[v], end = a.row_ptr[v + 1];
    unsigned long long qi = 0, qo = 0;
    uint32_t deg_in = 0;
    for (uint32_t d = beg; d < end; ++d) {
      const uint32_t x = a.ent[d];
      const double p = tf_project(a.dir_e, x >> 1, a0, a1, a2);
      const unsigned long long q = tf_weight(p);
      if ((p > 0.0) != ((x & 1u) != 0)) qo += q; else { qi += q; ++deg_in; }
    }
    S.qin[v] = qi; S.qout[v] = qo; S.indeg[v] = deg_in;
    S.pass[v] = end > beg ? GSFM_TF_LIVE : GSFM_TF_ABSENT;
    if (end > beg) {
      ++mine;
      if (deg_in == 0) S.list[atomicAdd(&n_new[0], 1u)] = v;
    }
  }
  for (uint32_t g = tid; g < G; g += nt) S.dirty[g] = 1u;
  if (mine) atomicAdd(&n_present, mine);
  __syncthreads();

  uint32_t live = n_present, head = 0, pass_no = 0, picks = 0;
  // (every pass removes a camera: at most `live` passes; the bound on pass_no only makes that visible)
  while (live > 0 && pass_no < n) {
    const uint32_t cnt = n_new[pass_no % 3];
    uint32_t* next_new = &n_new[(pass_no + 1) % 3];
    if (tid == 0) n_new[(pass_no + 2) % 3] = 0;   // read by the pass before this one, appended to by the pass after it
    if (cnt > 0) {
      // ---- source pass: the cameras list[head, head + cnt) go, one wavefront each (no two of them are neighbours) ----------------------
      const uint32_t base = head + cnt;
      for (uint32_t it = head + wave; it < base; it += n_waves) {
        const uint32_t u = S.list[it];
        if (lane == 0) { S.pass[u] = pass_no; S.dirty[u / GSFM_TF_GROUP] = 1u; }
        const uint32_t end = a.row_ptr[u + 1];
        for (uint32_t d = a.row_ptr[u] + lane; d < end; d += 64) tf_remove_entry(a, S, d, a0, a1, a2, base, next_new);
      }
      head = base; live -= cnt;
    } else {
      // ---- score pass: refresh the maxima of the groups a removal touched, pick the argmax over the groups, remove it --------------------
      for (uint32_t g = wave; g < G; g += n_waves) {
        if (!S.dirty[g]) continue;   // (wave-uniform)
        const uint32_t v = g * GSFM_TF_GROUP + lane;
        double s = -1.0; uint32_t i = 0xffffffffu;
        if (v < n && S.pass[v] == GSFM_TF_LIVE) { s = (double)(S.qout[v] + 4294967296ull) / (double)(S.qin[v] + 4294967296ull); i = v; }
        tf_wave_argmax(s, i);
        if (lane == 0) { S.gmax[g] = s; S.gidx[g] = i; S.dirty[g] = 0u; }
      }
      __syncthreads();
      double s = -1.0; uint32_t u = 0xffffffffu;
      for (uint32_t g = tid; g < G; g += nt) tf_better(s, u, S.gmax[g], S.gidx[g]);
      tf_wave_argmax(s, u);
      if (lane == 0) { red_s[wave] = s; red_i[wave] = u; }
      __syncthreads();
      s = red_s[0]; u = red_i[0];
      for (uint32_t w = 1; w < n_waves; ++w) tf_better(s, u, red_s[w], red_i[w]);
      if (u >= n) break;   // (cannot happen while a camera is live; uniform)
      if (tid == 0) { S.pass[u] = pass_no; S.dirty[u / GSFM_TF_GROUP] = 1u; }
      const uint32_t end = a.row_ptr[u + 1];
      for (uint32_t d = a.row_ptr[u] + tid; d < end; d += nt) tf_remove_entry(a, S, d, a0, a1, a2, head, next_new);
      live -= 1; ++picks;
    }
    ++pass_no;
    __syncthreads();
  }
  if (LDS) for (uint32_t v = tid; v < n; v += nt) a.pass_out[(size_t)k * n + v] = S.pass[v];
  if (tid == 0) { a.counts[2 * k] = pass_no; a.counts[2 * k + 1] = picks; }
}

// bad_e = sum_k [arc's tail removed in a later pass than its head] |p_ek|, k ascending; keep_e = !(bad_e > threshold)
__global__ void __launch_bounds__(256) k_tf_bad(uint32_t n_edges, uint32_t n_cams, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej,
                                                const double* __restrict__ dir_e, const double* __restrict__ axes, int n_axes,
                                                const uint32_t* __restrict__ pass, double threshold, double* __restrict__ bad_out,
                                                uint8_t* __restrict__ keep_out, unsigned long long* n_kept) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (e < n_edges) {
    const uint32_t i = ei[e], j = ej[e];
    double bad = 0.0;
    for (int k = 0; k < n_axes; ++k) {
      const double p = tf_project(dir_e, e, axes[3 * k], axes[3 * k + 1], axes[3 * k + 2]);
      const uint32_t pi = pass[(size_t)k * n_cams + i], pj = pass[(size_t)k * n_cams + j];
      if (p > 0.0 ? pi > pj : pj > pi) bad += fabs(p);
    }
    keep = !(bad > threshold);
    bad_out[e] = bad;
    keep_out[e] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_kept, (unsigned long long)__popcll(m));
}

}  // namespace gsfm
