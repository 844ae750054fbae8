// Host side of gsfm_rot_init_spanning_tree (include/gsfm_rot.h): validation, one device slab, the launch sequence of tree_kernels.hpp.
// Part of libgsfm_rot.so's one translation unit (included from gsfm_rot.hip after host_common.hpp).
#pragma once
#include "host_common.hpp"
#include "tree_kernels.hpp"

namespace {

inline int ceil_log2(uint64_t x) { int r = 0; while ((1ull << r) < x) ++r; return r; }

// The first bad edge, or -1: an out-of-range camera or a self-loop.  Threads over contiguous ranges; the smallest index is reported.
int64_t first_bad_edge(uint32_t n_cams, uint64_t n_edges, const uint32_t* ei, const uint32_t* ej) {
  const int T = n_edges >= (1u << 20) ? host_threads() : 1;
  std::vector<int64_t> bad((size_t)T, -1);
  parallel_run(T, [&](int t, int TT) {
    const uint64_t lo = n_edges * t / TT, hi = n_edges * (t + 1) / TT;
    for (uint64_t e = lo; e < hi; ++e)
      if (ei[e] >= n_cams || ej[e] >= n_cams || ei[e] == ej[e]) { bad[t] = (int64_t)e; return; }
  });
  for (int64_t b : bad) if (b >= 0) return b;
  return -1;
}

gsfm_status init_spanning_tree_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                                    const int32_t* weight, double* rot_aa_out, int64_t* parent_edge_out, uint32_t* root_out,
                                    uint32_t* n_tree_cams_out, uint32_t* depth_out, double* kernel_ms) {
  if (!rot_aa_out || (n_edges > 0 && (!edge_i || !edge_j || !rel_aa))) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 32)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "gsfm_rot_init_spanning_tree takes fewer than 2^32 edges");
  if (n_cams >= 0x7fffffffu) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "gsfm_rot_init_spanning_tree takes fewer than 2^31 - 1 cameras");
  const int64_t bad = first_bad_edge(n_cams, n_edges, edge_i, edge_j);
  if (bad >= 0)
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(bad) + " has an out-of-range camera index or joins a camera to itself");
  const size_t N = n_cams;
  auto empty_outputs = [&]() {
    std::memset(rot_aa_out, 0, 24 * N);
    if (parent_edge_out) for (size_t v = 0; v < N; ++v) parent_edge_out[v] = -1;
  };
  if (n_edges == 0) {   // every component is one camera: nothing to initialise (the host knows without a device)
    empty_outputs();
    return (gsfm_status)fail(GSFM_ERR_EMPTY, "the largest connected component has one camera");
  }
  if (const char* why = no_device_reason("the spanning-tree initialisation")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  // One device slab, one private stream, stream-ordered copies, no hipDeviceSynchronize; the guard owns everything on every path.
  struct Guard {
    hipStream_t s = nullptr; hipEvent_t ev[6] = {}; void* slab = nullptr;
    ~Guard() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); if (slab) (void)hipFree(slab); if (s) (void)hipStreamDestroy(s); }
  } G;
  const size_t E = n_edges;
  const int R = ceil_log2(N) + 1;   // Boruvka rounds: the components that still have an outgoing edge at least halve every round
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up(bytes); return o; };
  const size_t o_i = take(4 * E), o_j = take(4 * E), o_w = weight ? take(4 * E) : 0, o_recA = take(16 * E), o_recB = take(16 * E),
               o_cnt = take(4 * (size_t)(R + 2)), o_comp = take(4 * N), o_par = take(4 * N), o_best = take(8 * N), o_size = take(4 * N),
               o_minv = take(4 * N), o_forest = take(4 * N), o_pick = take(8), o_sc = take(16), o_tlist = take(4 * N), o_head = take(4 * N),
               o_link = take(8 * N), o_nxt0 = take(8 * N), o_nxt1 = take(8 * N), o_dist0 = take(8 * N), o_dist1 = take(8 * N),
               o_P0 = take(4 * N), o_P1 = take(4 * N), o_D0 = take(4 * N), o_D1 = take(4 * N), o_A0 = take(32 * N), o_A1 = take(32 * N),
               o_pe = take(4 * N), o_rel = take(24 * N), o_rot = take(24 * N), o_pout = take(8 * N), o_maxd = take(4), total = off;
  HIPCHK_S(hipStreamCreateWithFlags(&G.s, hipStreamNonBlocking));
  for (hipEvent_t& e : G.ev) HIPCHK_S(hipEventCreate(&e));
  if (hipMalloc(&G.slab, total) != hipSuccess) { G.slab = nullptr; return (gsfm_status)fail(GSFM_ERR_HIP, "allocating the spanning-tree buffers failed"); }
  char* base = (char*)G.slab;
  auto U = [&](size_t o) { return (uint32_t*)(base + o); };
  const hipStream_t s = G.s;
  // 12 B per edge go up (the relative rotations of the n_c - 1 tree edges follow once the tree is known)
  HIPCHK_S(hipMemcpyAsync(base + o_i, edge_i, 4 * E, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_j, edge_j, 4 * E, hipMemcpyHostToDevice, s));
  if (weight) HIPCHK_S(hipMemcpyAsync(base + o_w, weight, 4 * E, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemsetAsync(base + o_cnt, 0, 4 * (size_t)(R + 2), s));
  HIPCHK_S(hipMemsetAsync(base + o_best, 0, 8 * N, s));
  HIPCHK_S(hipMemsetAsync(base + o_size, 0, 4 * N, s));
  HIPCHK_S(hipMemsetAsync(base + o_minv, 0xff, 4 * N, s));
  HIPCHK_S(hipMemsetAsync(base + o_head, 0xff, 4 * N, s));
  HIPCHK_S(hipMemsetAsync(base + o_pick, 0, 8, s));
  HIPCHK_S(hipMemsetAsync(base + o_sc, 0, 16, s));
  HIPCHK_S(hipMemsetAsync(base + o_maxd, 0, 4, s));
  const uint32_t* ei = U(o_i); const uint32_t* ej = U(o_j);
  const int32_t* w = weight ? (const int32_t*)(base + o_w) : nullptr;
  uint32_t* cnt = U(o_cnt); uint32_t* comp = U(o_comp); uint32_t* par = U(o_par); uint32_t* sc = U(o_sc);
  unsigned long long* best = (unsigned long long*)(base + o_best);
  MstEdge* rec[2] = {(MstEdge*)(base + o_recA), (MstEdge*)(base + o_recB)};
  const dim3 blk(256), gN(grid_for(N)), gE((unsigned)std::min<size_t>(grid_for(E), 4096));

  // ---- phase 1: the maximum spanning forest, the largest component, its tree edges --------------------------------------------------
  HIPCHK_S(hipEventRecord(G.ev[0], s));
  hipLaunchKernelGGL(k_mst_init, gN, blk, 0, s, n_cams, comp);
  for (int r = 0; r <= R; ++r) {   // round R only counts the edges that still join two components: none, or the rounds were too few
    hipLaunchKernelGGL(k_mst_propose, gE, blk, 0, s, ei, ej, w, (uint64_t)E, r ? (const MstEdge*)rec[(r - 1) & 1] : nullptr, r ? (const uint32_t*)(cnt + r - 1) : nullptr,
                       (const uint32_t*)comp, best, rec[r & 1], cnt + r);
    if (r == R) break;
    hipLaunchKernelGGL(k_mst_hook, gN, blk, 0, s, n_cams, ei, ej, (const uint32_t*)comp, (const unsigned long long*)best, par, U(o_forest), cnt + R + 1);
    hipLaunchKernelGGL(k_mst_jump, gN, blk, 0, s, n_cams, comp, par, best);
  }
  hipLaunchKernelGGL(k_comp_count, gN, blk, 0, s, n_cams, (const uint32_t*)comp, U(o_size), U(o_minv));
  hipLaunchKernelGGL(k_comp_pick, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)U(o_size), (const uint32_t*)U(o_minv), (unsigned long long*)(base + o_pick));
  hipLaunchKernelGGL(k_comp_chosen, dim3(1), dim3(1), 0, s, (const uint32_t*)comp, (const unsigned long long*)(base + o_pick), sc);
  hipLaunchKernelGGL(k_tree_list, gN, blk, 0, s, (const uint32_t*)U(o_forest), (const uint32_t*)(cnt + R + 1), ei, ej, (const uint32_t*)comp, sc, U(o_tlist), U(o_head), U(o_link));
  HIPCHK_S(hipEventRecord(G.ev[1], s));
  std::vector<uint32_t> h_cnt((size_t)R + 2), h_sc(4), tlist(N);
  HIPCHK_S(hipMemcpyAsync(h_cnt.data(), cnt, 4 * (size_t)(R + 2), hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipMemcpyAsync(h_sc.data(), sc, 16, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipMemcpyAsync(tlist.data(), U(o_tlist), 4 * N, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipStreamSynchronize(s));
  HIPCHK_S(hipGetLastError());
  if (h_cnt[R] != 0) return (gsfm_status)fail(GSFM_ERR_HIP, "spanning tree: edges between components remain after the last Boruvka round");
  const uint32_t root = h_sc[1], n_c = h_sc[2], m = h_sc[3];
  if (n_c < 2) { empty_outputs(); return (gsfm_status)fail(GSFM_ERR_EMPTY, "the largest connected component has one camera"); }
  if (m != n_c - 1 || root >= n_cams) return (gsfm_status)fail(GSFM_ERR_HIP, "spanning tree: the chosen component's tree is inconsistent");

  // ---- phase 2: root the tree (Euler tour, list ranking) while the host gathers the tree edges' relative rotations ------------------
  const dim3 gD(grid_for(2 * (size_t)m)), gM(grid_for(m));
  uint32_t* nxt[2] = {U(o_nxt0), U(o_nxt1)}; uint32_t* dist[2] = {U(o_dist0), U(o_dist1)};
  HIPCHK_S(hipEventRecord(G.ev[2], s));
  hipLaunchKernelGGL(k_tree_tour, gD, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)U(o_tlist), ei, ej, (const uint32_t*)U(o_head), (const uint32_t*)U(o_link), nxt[0], dist[0]);
  const int RR = ceil_log2(2 * (uint64_t)m);
  for (int r = 0; r < RR; ++r)
    hipLaunchKernelGGL(k_tree_rank, gD, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)nxt[r & 1], (const uint32_t*)dist[r & 1], nxt[(r + 1) & 1], dist[(r + 1) & 1]);
  HIPCHK_S(hipEventRecord(G.ev[3], s));
  std::vector<double> rel((size_t)3 * m);
  for (uint32_t k = 0; k < m; ++k) { const double* a = rel_aa + 3 * (size_t)tlist[k]; rel[3 * (size_t)k] = a[0]; rel[3 * (size_t)k + 1] = a[1]; rel[3 * (size_t)k + 2] = a[2]; }
  HIPCHK_S(hipMemcpyAsync(base + o_rel, rel.data(), 24 * (size_t)m, hipMemcpyHostToDevice, s));

  // ---- phase 3: orient, compose by pointer doubling, write out -------------------------------------------------------------------
  uint32_t* P[2] = {U(o_P0), U(o_P1)}; uint32_t* D[2] = {U(o_D0), U(o_D1)}; Quat* A[2] = {(Quat*)(base + o_A0), (Quat*)(base + o_A1)};
  HIPCHK_S(hipEventRecord(G.ev[4], s));
  hipLaunchKernelGGL(k_tree_orient, gM, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)U(o_tlist), ei, ej, (const uint32_t*)dist[RR & 1], (const double*)(base + o_rel),
                     P[0], D[0], A[0], U(o_pe));
  const int RD = ceil_log2(n_c);
  for (int r = 0; r < RD; ++r)
    hipLaunchKernelGGL(k_tree_double, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)sc, (const uint32_t*)P[r & 1], (const uint32_t*)D[r & 1],
                       (const Quat*)A[r & 1], P[(r + 1) & 1], D[(r + 1) & 1], A[(r + 1) & 1]);
  hipLaunchKernelGGL(k_tree_out, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)sc, (const Quat*)A[RD & 1], (const uint32_t*)D[RD & 1],
                     (const uint32_t*)U(o_pe), (const uint32_t*)U(o_tlist), (double*)(base + o_rot), (long long*)(base + o_pout), U(o_maxd));
  HIPCHK_S(hipEventRecord(G.ev[5], s));
  uint32_t maxd = 0;
  HIPCHK_S(hipMemcpyAsync(rot_aa_out, base + o_rot, 24 * N, hipMemcpyDeviceToHost, s));
  if (parent_edge_out) HIPCHK_S(hipMemcpyAsync(parent_edge_out, base + o_pout, 8 * N, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipMemcpyAsync(&maxd, U(o_maxd), 4, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipStreamSynchronize(s));
  HIPCHK_S(hipGetLastError());
  if (kernel_ms) {
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, G.ev[0], G.ev[1]); (void)hipEventElapsedTime(&b, G.ev[2], G.ev[3]); (void)hipEventElapsedTime(&c, G.ev[4], G.ev[5]);
    *kernel_ms = (double)a + b + c;
  }
  if (root_out) *root_out = root;
  if (n_tree_cams_out) *n_tree_cams_out = n_c;
  if (depth_out) *depth_out = maxd;
  return GSFM_OK;
}

}  // namespace
