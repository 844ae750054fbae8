// Kernels of the maximum-spanning-tree initialisation (gsfm_rot_init_spanning_tree; host side: spanning_tree.hpp).
//
// Edge order.  key(e) = ((uint32)(w ^ INT32_MIN) << 32) | (uint32)~e: a larger weight wins, on equal weights the smaller edge index.
// The keys are distinct, so the maximum spanning forest is unique and every step below is free to run in any order.  Key 0 is never
// a real edge (it would need e = 2^32 - 1, and the host rejects n_edges >= 2^32): it marks "no proposal".
//
// 1. Boruvka rounds (k_mst_propose, k_mst_hook, k_mst_jump), all labels are stars (comp[v] = root label) between rounds:
//    propose  every edge between two components does an integer atomicMax of its key into best[] of both ends, after a plain load
//             shows it can win (values only grow, so a stale load costs at most one needless atomic); a wavefront whose live lanes
//             share one destination reduces first and sends one atomic.  The edges whose two ends already share a label are dropped:
//             the survivors are appended to the next round's list (order irrelevant: max is order-free).
//    hook     each root follows its best edge to the other component; the only cycles are 2-cycles over one edge, broken by the
//             smaller label staying root.  The hooking root appends the edge to the forest list, so each tree edge is listed once.
//    jump     labels follow the hook forest to its roots by in-place path halving.  A thread only ever replaces par[r] by an
//             ancestor of r, so every value it reads, however stale, is an ancestor: each step moves up, nothing waits on anyone.
// 2. Largest component (k_comp_count, k_comp_pick): sizes by integer atomics and the per-label minimum camera, then one 64-bit max of
//    (size, ~min camera): the largest component, ties to the one holding the smallest camera.  Its root is that smallest camera.
// 3. Rooting (k_tree_*): Euler tour of the chosen tree.  Adjacency lists are linked lists built with atomicExch (head / link); the
//    successor of the directed edge u->v is the edge after v->u in v's cyclic list.  The tour is cut in front of the root's first
//    edge and ranked by pointer jumping (Wyllie, ping-pong buffers, a fixed number of rounds); of the two directions of a tree edge
//    the one with the larger distance to the end of the tour points away from the root.
// 4. Composition (k_tree_double): R_v = A_v R_P(v), A_v = the edge's relative rotation to start with, then pointer doubling
//    A_v <- A_v A_P(v), D_v <- D_v + D_P(v), P(v) <- P(P(v)) for ceil(log2 n_c) rounds, quaternions throughout, one conversion to
//    angle-axis at the end.  The products are grouped by the tree alone, so two calls give the same bits.
// No float atomics, no spin or wait on another workgroup anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so3_dev.hpp"

namespace gsfm {

#define GSFM_TREE_NONE 0xffffffffu

struct MstEdge { uint32_t a, b; unsigned long long key; };   // 16 B survivor record

__device__ __forceinline__ unsigned long long mst_key(int32_t w, uint32_t e) {
  return ((unsigned long long)((uint32_t)w ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)~e;
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One proposal per lane (act = the lane has one).  Called by every lane of the wavefront (the loops below keep waves uniform).
__device__ __forceinline__ void mst_offer(unsigned long long* best, uint32_t c, unsigned long long key, bool act) {
  const unsigned long long live = __ballot(act);
  if (live == 0) return;
  const int lead = __ffsll((long long)live) - 1;
  const uint32_t c0 = __shfl(c, lead, 64);
  if (__all(!act || c == c0)) {   // one destination for the whole wave: reduce, then one atomic
    unsigned long long k = act ? key : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(k, off, 64); k = o > k ? o : k; }
    if ((int)(threadIdx.x & 63) == lead && k > __hip_atomic_load(best + c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(best + c0, k);
    return;
  }
  if (act && key > __hip_atomic_load(best + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(best + c, key);
}

__global__ void __launch_bounds__(256) k_mst_init(uint32_t n, uint32_t* comp) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) comp[v] = v;
}

// Round 0 reads the caller's arrays (w == nullptr: all weights equal); later rounds the survivor list of the round before.
__global__ void __launch_bounds__(256) k_mst_propose(const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej, const int32_t* __restrict__ w,
                                                     uint64_t n_first, const MstEdge* __restrict__ in, const uint32_t* n_in,
                                                     const uint32_t* __restrict__ comp, unsigned long long* best, MstEdge* __restrict__ out, uint32_t* n_out) {
  const uint64_t n = in ? (uint64_t)*n_in : n_first;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += stride) {   // wave-uniform trip count
    const uint64_t i = base + threadIdx.x;
    MstEdge r{0u, 0u, 0ull};
    if (i < n) {
      if (in) r = in[i];
      else { r.a = ei[i]; r.b = ej[i]; r.key = mst_key(w ? w[i] : 0, (uint32_t)i); }
    }
    const uint32_t cu = i < n ? comp[r.a] : 0u, cv = i < n ? comp[r.b] : 0u;
    const bool live = i < n && cu != cv;
    if (live) out[atomicAdd(n_out, 1u)] = r;
    mst_offer(best, cu, r.key, live);
    mst_offer(best, cv, r.key, live);
  }
}

__global__ void __launch_bounds__(256) k_mst_hook(uint32_t n, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej, const uint32_t* __restrict__ comp,
                                                  const unsigned long long* __restrict__ best, uint32_t* par, uint32_t* forest, uint32_t* n_forest) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || comp[v] != v) return;
  const unsigned long long b = best[v];
  if (b == 0ull) { par[v] = v; return; }
  const uint32_t e = ~(uint32_t)b;
  const uint32_t cu = comp[ei[e]], cv = comp[ej[e]];
  const uint32_t other = cu == v ? cv : cu;
  if (best[other] == b && v < other) { par[v] = v; return; }   // 2-cycle over edge e: the smaller label stays root
  par[v] = other;
  forest[atomicAdd(n_forest, 1u)] = e;
}

__global__ void __launch_bounds__(256) k_mst_jump(uint32_t n, uint32_t* comp, uint32_t* par, unsigned long long* best) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  uint32_t r = comp[v];
  for (;;) {   // path halving; every iteration moves r strictly up the hook forest
    const uint32_t p = ld_agent(par + r);
    if (p == r) break;
    const uint32_t pp = ld_agent(par + p);
    if (pp == p) { r = p; break; }
    st_agent(par + r, pp);
    r = pp;
  }
  comp[v] = r;
  best[v] = 0ull;
}

// Component sizes and minimum cameras; a wavefront whose cameras share one label sends one add and one min.
__global__ void __launch_bounds__(256) k_comp_count(uint32_t n, const uint32_t* __restrict__ comp, uint32_t* size, uint32_t* minv) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = v < n;
  const uint32_t c = act ? comp[v] : 0u;
  const unsigned long long live = __ballot(act);
  if (live == 0) return;
  const int lead = __ffsll((long long)live) - 1;
  const uint32_t c0 = __shfl(c, lead, 64);
  if (__all(!act || c == c0)) {
    if ((int)(threadIdx.x & 63) == lead) { atomicAdd(size + c0, (uint32_t)__popcll(live)); atomicMin(minv + c0, v); }   // lead = smallest camera of the wave
    return;
  }
  if (act) { atomicAdd(size + c, 1u); atomicMin(minv + c, v); }
}

__global__ void __launch_bounds__(256) k_comp_pick(uint32_t n, const uint32_t* __restrict__ comp, const uint32_t* __restrict__ size, const uint32_t* __restrict__ minv,
                                                   unsigned long long* pick) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || comp[v] != v) return;
  const unsigned long long k = ((unsigned long long)size[v] << 32) | (unsigned long long)(uint32_t)~minv[v];
  if (k > __hip_atomic_load(pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(pick, k);
}

// Scalars of the chosen component, written by one thread: [0] label, [1] root camera, [2] size, [3] tree edges listed (k_tree_list)
__global__ void k_comp_chosen(const uint32_t* __restrict__ comp, const unsigned long long* __restrict__ pick, uint32_t* sc) {
  const uint32_t root = ~(uint32_t)*pick;
  sc[0] = comp[root]; sc[1] = root; sc[2] = (uint32_t)(*pick >> 32);
}

// The forest edges inside the chosen component; both directions get their place in the adjacency lists.
__global__ void __launch_bounds__(256) k_tree_list(const uint32_t* __restrict__ forest, const uint32_t* n_forest, const uint32_t* __restrict__ ei,
                                                   const uint32_t* __restrict__ ej, const uint32_t* __restrict__ comp, uint32_t* sc, uint32_t* tlist,
                                                   uint32_t* head, uint32_t* link) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= *n_forest) return;
  const uint32_t e = forest[f], a = ei[e], b = ej[e];
  if (comp[a] != sc[0]) return;
  const uint32_t k = atomicAdd(sc + 3, 1u);
  tlist[k] = e;
  link[2 * k] = atomicExch(head + a, 2 * k);          // 2k: a -> b, out of a
  link[2 * k + 1] = atomicExch(head + b, 2 * k + 1);  // 2k + 1: b -> a, out of b
}

// Tour successor of every directed tree edge, cut in front of the root's first edge; dist = 1 except at the cut (0).
__global__ void __launch_bounds__(256) k_tree_tour(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ tlist, const uint32_t* __restrict__ ei,
                                                   const uint32_t* __restrict__ ej, const uint32_t* __restrict__ head, const uint32_t* __restrict__ link,
                                                   uint32_t* nxt, uint32_t* dist) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= 2 * sc[3]) return;
  const uint32_t e = tlist[d >> 1];
  const uint32_t v = (d & 1) ? ei[e] : ej[e];   // head of d
  const uint32_t r = d ^ 1u;                    // v -> (tail of d), out of v
  const uint32_t s = link[r] != GSFM_TREE_NONE ? link[r] : head[v];
  const bool cut = s == head[sc[1]];
  nxt[d] = cut ? GSFM_TREE_NONE : s;
  dist[d] = cut ? 0u : 1u;
}

__global__ void __launch_bounds__(256) k_tree_rank(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ nxt, const uint32_t* __restrict__ dist,
                                                   uint32_t* nxt_out, uint32_t* dist_out) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= 2 * sc[3]) return;
  const uint32_t s = nxt[d];
  nxt_out[d] = s == GSFM_TREE_NONE ? s : nxt[s];
  dist_out[d] = s == GSFM_TREE_NONE ? dist[d] : dist[d] + dist[s];
}

// Parent, tree edge and relative rotation of every camera of the component (rel: the tree edges' angle-axis, tree-edge order).
__global__ void __launch_bounds__(256) k_tree_orient(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ tlist, const uint32_t* __restrict__ ei,
                                                     const uint32_t* __restrict__ ej, const uint32_t* __restrict__ dist, const double* __restrict__ rel,
                                                     uint32_t* P, uint32_t* D, Quat* A, uint32_t* pe) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) { const uint32_t root = sc[1]; P[root] = root; D[root] = 0u; A[root] = Quat{0.0, 0.0, 0.0, 1.0}; pe[root] = GSFM_TREE_NONE; }
  if (k >= sc[3]) return;
  const uint32_t e = tlist[k], a = ei[e], b = ej[e];
  const Quat q = aa_to_quat(rel[3 * (size_t)k], rel[3 * (size_t)k + 1], rel[3 * (size_t)k + 2]);   // R_ab: R_b = R_ab R_a
  const bool down = dist[2 * k] > dist[2 * k + 1];   // a -> b points away from the root
  const uint32_t child = down ? b : a;
  P[child] = down ? a : b;
  D[child] = 1u;
  A[child] = down ? q : qconj(q);
  pe[child] = k;
}

__global__ void __launch_bounds__(256) k_tree_double(uint32_t n, const uint32_t* __restrict__ comp, const uint32_t* __restrict__ sc,
                                                     const uint32_t* __restrict__ P, const uint32_t* __restrict__ D, const Quat* __restrict__ A,
                                                     uint32_t* P_out, uint32_t* D_out, Quat* A_out) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || comp[v] != sc[0]) return;
  const uint32_t p = P[v];
  A_out[v] = qmul(A[v], A[p]);
  D_out[v] = D[v] + D[p];
  P_out[v] = P[p];
}

__global__ void __launch_bounds__(256) k_tree_out(uint32_t n, const uint32_t* __restrict__ comp, const uint32_t* __restrict__ sc, const Quat* __restrict__ A,
                                                  const uint32_t* __restrict__ D, const uint32_t* __restrict__ pe, const uint32_t* __restrict__ tlist,
                                                  double* rot, long long* parent_edge, uint32_t* max_depth) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  double a[3] = {0.0, 0.0, 0.0};
  long long pv = -1;
  if (comp[v] == sc[0]) {
    if (v != sc[1]) {
      double s, t;
      quat_log(A[v], a, &s, &t);
      pv = (long long)tlist[pe[v]];
    }
    atomicMax(max_depth, D[v]);
  }
  rot[3 * (size_t)v] = a[0]; rot[3 * (size_t)v + 1] = a[1]; rot[3 * (size_t)v + 2] = a[2];
  parent_edge[v] = pv;
}

}  // namespace gsfm
