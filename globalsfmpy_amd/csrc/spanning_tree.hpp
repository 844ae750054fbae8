// Host side of gsfm_rot_init_spanning_tree (include/gsfm_rot.h): validation, one device slab (flat_call.hpp), the launch sequence of tree_kernels.hpp.
// Part of libgsfm_rot.so's one translation unit (included from gsfm_rot.hip after host_common.hpp).
#pragma once
#include "flat_call.hpp"
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

  const size_t E = n_edges;
  const int R = ceil_log2(N) + 1;   // Boruvka rounds: the components that still have an outgoing edge at least halve every round
  FlatLayout L;
  const auto s_i = L.take<uint32_t>(E), s_j = L.take<uint32_t>(E); const auto s_w = L.take<int32_t>(weight ? E : 0);
  const auto s_recA = L.take<MstEdge>(E), s_recB = L.take<MstEdge>(E);
  const auto s_cnt = L.take<uint32_t>((size_t)(R + 2)), s_comp = L.take<uint32_t>(N), s_par = L.take<uint32_t>(N); const auto s_best = L.take<unsigned long long>(N);
  const auto s_size = L.take<uint32_t>(N), s_minv = L.take<uint32_t>(N), s_forest = L.take<uint32_t>(N); const auto s_pick = L.take<unsigned long long>(1);
  const auto s_sc = L.take<uint32_t>(4), s_tlist = L.take<uint32_t>(N), s_head = L.take<uint32_t>(N), s_link = L.take<uint32_t>(2 * N),
             s_nxt0 = L.take<uint32_t>(2 * N), s_nxt1 = L.take<uint32_t>(2 * N), s_dist0 = L.take<uint32_t>(2 * N), s_dist1 = L.take<uint32_t>(2 * N),
             s_P0 = L.take<uint32_t>(N), s_P1 = L.take<uint32_t>(N), s_D0 = L.take<uint32_t>(N), s_D1 = L.take<uint32_t>(N);
  const auto s_A0 = L.take<Quat>(N), s_A1 = L.take<Quat>(N); const auto s_pe = L.take<uint32_t>(N);
  const auto s_rel = L.take<double>(3 * N), s_rot = L.take<double>(3 * N); const auto s_pout = L.take<long long>(N); const auto s_maxd = L.take<uint32_t>(1);
  FlatCall fc;
  if (int st = fc.commit(L, "the spanning-tree initialisation", 3)) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  // 12 B per edge go up (the relative rotations of the n_c - 1 tree edges follow once the tree is known)
  HIPCHK_S(fc.upload(s_i, edge_i, E)); HIPCHK_S(fc.upload(s_j, edge_j, E));
  if (weight) HIPCHK_S(fc.upload(s_w, weight, E));
  HIPCHK_S(fc.zero(s_cnt, (size_t)(R + 2))); HIPCHK_S(fc.zero(s_best, N)); HIPCHK_S(fc.zero(s_size, N));
  HIPCHK_S(hipMemsetAsync(fc.ptr(s_minv), 0xff, 4 * N, s)); HIPCHK_S(hipMemsetAsync(fc.ptr(s_head), 0xff, 4 * N, s));
  HIPCHK_S(fc.zero(s_pick, 1)); HIPCHK_S(fc.zero(s_sc, 4)); HIPCHK_S(fc.zero(s_maxd, 1));
  const uint32_t* ei = fc.ptr(s_i); const uint32_t* ej = fc.ptr(s_j);
  const int32_t* w = weight ? fc.ptr(s_w) : nullptr;
  uint32_t* cnt = fc.ptr(s_cnt); uint32_t* comp = fc.ptr(s_comp); uint32_t* par = fc.ptr(s_par); uint32_t* sc = fc.ptr(s_sc);
  unsigned long long* best = fc.ptr(s_best);
  MstEdge* rec[2] = {fc.ptr(s_recA), fc.ptr(s_recB)};
  uint32_t* size = fc.ptr(s_size); uint32_t* minv = fc.ptr(s_minv); uint32_t* forest = fc.ptr(s_forest); uint32_t* tlist_d = fc.ptr(s_tlist);
  uint32_t* head = fc.ptr(s_head); uint32_t* link = fc.ptr(s_link); uint32_t* pe = fc.ptr(s_pe);
  const dim3 blk(256), gN(grid_for(N)), gE((unsigned)std::min<size_t>(grid_for(E), 4096));

  // ---- phase 1: the maximum spanning forest, the largest component, its tree edges --------------------------------------------------
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_mst_init, gN, blk, 0, s, n_cams, comp);
  for (int r = 0; r <= R; ++r) {   // round R only counts the edges that still join two components: none, or the rounds were too few
    hipLaunchKernelGGL(k_mst_propose, gE, blk, 0, s, ei, ej, w, (uint64_t)E, r ? (const MstEdge*)rec[(r - 1) & 1] : nullptr, r ? (const uint32_t*)(cnt + r - 1) : nullptr,
                       (const uint32_t*)comp, best, rec[r & 1], cnt + r);
    if (r == R) break;
    hipLaunchKernelGGL(k_mst_hook, gN, blk, 0, s, n_cams, ei, ej, (const uint32_t*)comp, (const unsigned long long*)best, par, forest, cnt + R + 1);
    hipLaunchKernelGGL(k_mst_jump, gN, blk, 0, s, n_cams, comp, par, best);
  }
  hipLaunchKernelGGL(k_comp_count, gN, blk, 0, s, n_cams, (const uint32_t*)comp, size, minv);
  hipLaunchKernelGGL(k_comp_pick, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)size, (const uint32_t*)minv, fc.ptr(s_pick));
  hipLaunchKernelGGL(k_comp_chosen, dim3(1), dim3(1), 0, s, (const uint32_t*)comp, (const unsigned long long*)fc.ptr(s_pick), sc);
  hipLaunchKernelGGL(k_tree_list, gN, blk, 0, s, (const uint32_t*)forest, (const uint32_t*)(cnt + R + 1), ei, ej, (const uint32_t*)comp, sc, tlist_d, head, link);
  HIPCHK_S(fc.end_span());
  std::vector<uint32_t> h_cnt((size_t)R + 2), h_sc(4), tlist(N);
  HIPCHK_S(fc.download(h_cnt.data(), s_cnt, (size_t)(R + 2)));
  HIPCHK_S(fc.download(h_sc.data(), s_sc, 4));
  HIPCHK_S(fc.download(tlist.data(), s_tlist, N));
  HIPCHK_S(fc.sync());
  if (h_cnt[R] != 0) return (gsfm_status)fail(GSFM_ERR_HIP, "spanning tree: edges between components remain after the last Boruvka round");
  const uint32_t root = h_sc[1], n_c = h_sc[2], m = h_sc[3];
  if (n_c < 2) { empty_outputs(); return (gsfm_status)fail(GSFM_ERR_EMPTY, "the largest connected component has one camera"); }
  if (m != n_c - 1 || root >= n_cams) return (gsfm_status)fail(GSFM_ERR_HIP, "spanning tree: the chosen component's tree is inconsistent");

  // ---- phase 2: root the tree (Euler tour, list ranking) while the host gathers the tree edges' relative rotations ------------------
  const dim3 gD(grid_for(2 * (size_t)m)), gM(grid_for(m));
  uint32_t* nxt[2] = {fc.ptr(s_nxt0), fc.ptr(s_nxt1)}; uint32_t* dist[2] = {fc.ptr(s_dist0), fc.ptr(s_dist1)};
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_tree_tour, gD, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)tlist_d, ei, ej, (const uint32_t*)head, (const uint32_t*)link, nxt[0], dist[0]);
  const int RR = ceil_log2(2 * (uint64_t)m);
  for (int r = 0; r < RR; ++r)
    hipLaunchKernelGGL(k_tree_rank, gD, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)nxt[r & 1], (const uint32_t*)dist[r & 1], nxt[(r + 1) & 1], dist[(r + 1) & 1]);
  HIPCHK_S(fc.end_span());
  std::vector<double> rel((size_t)3 * m);
  for (uint32_t k = 0; k < m; ++k) { const double* a = rel_aa + 3 * (size_t)tlist[k]; rel[3 * (size_t)k] = a[0]; rel[3 * (size_t)k + 1] = a[1]; rel[3 * (size_t)k + 2] = a[2]; }
  HIPCHK_S(fc.upload(s_rel, rel.data(), 3 * (size_t)m));

  // ---- phase 3: orient, compose by pointer doubling, write out -------------------------------------------------------------------
  uint32_t* P[2] = {fc.ptr(s_P0), fc.ptr(s_P1)}; uint32_t* D[2] = {fc.ptr(s_D0), fc.ptr(s_D1)}; Quat* A[2] = {fc.ptr(s_A0), fc.ptr(s_A1)};
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_tree_orient, gM, blk, 0, s, (const uint32_t*)sc, (const uint32_t*)tlist_d, ei, ej, (const uint32_t*)dist[RR & 1], (const double*)fc.ptr(s_rel),
                     P[0], D[0], A[0], pe);
  const int RD = ceil_log2(n_c);
  for (int r = 0; r < RD; ++r)
    hipLaunchKernelGGL(k_tree_double, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)sc, (const uint32_t*)P[r & 1], (const uint32_t*)D[r & 1],
                       (const Quat*)A[r & 1], P[(r + 1) & 1], D[(r + 1) & 1], A[(r + 1) & 1]);
  hipLaunchKernelGGL(k_tree_out, gN, blk, 0, s, n_cams, (const uint32_t*)comp, (const uint32_t*)sc, (const Quat*)A[RD & 1], (const uint32_t*)D[RD & 1],
                     (const uint32_t*)pe, (const uint32_t*)tlist_d, fc.ptr(s_rot), fc.ptr(s_pout), fc.ptr(s_maxd));
  HIPCHK_S(fc.end_span());
  uint32_t maxd = 0;
  HIPCHK_S(fc.download(rot_aa_out, s_rot, 3 * N));
  if (parent_edge_out) HIPCHK_S(fc.download(parent_edge_out, s_pout, N));
  HIPCHK_S(fc.download(&maxd, s_maxd, 1));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  if (root_out) *root_out = root;
  if (n_tree_cams_out) *n_tree_cams_out = n_c;
  if (depth_out) *depth_out = maxd;
  return GSFM_OK;
}

}  // namespace
