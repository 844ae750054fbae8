// Host side of gsfm_pos_refine_relative_translations (include/gsfm_pos.h): validation, the launch order (edges by descending match
// count), one device slab (flat_call.hpp) and the one launch of trans_refine_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "flat_call.hpp"
#include "trans_refine_kernels.hpp"
#include "../../include/gsfm_pos.h"

namespace {

gsfm_status trans_refine_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr,
                              const double* matches, const double* intrinsics, const double* rot_aa, const double* rel_t_in, double* rel_t_out,
                              int32_t* status_out, int32_t* iters_out, double* cost_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_edges == 0) return GSFM_OK;   // nothing to refine
  if (!edge_i || !edge_j || !match_ptr || !intrinsics || !rot_aa || !rel_t_in || !rel_t_out || !status_out)
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges)");
  for (uint64_t e = 0; e < n_edges; ++e) {
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams)
      return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has an out-of-range camera index");
    if (match_ptr[e + 1] < match_ptr[e]) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "match_ptr decreases at edge " + std::to_string(e));
  }
  const size_t E = n_edges, N = n_cams, M = match_ptr[E];
  if (M > 0 && !matches) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (const char* why = no_device_reason("the translation refinement")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  // launch order: descending match count, equal counts by edge index -- the long edges start first and neighbours in the grid are alike
  hvec<uint32_t> order(E);
  for (size_t e = 0; e < E; ++e) order[e] = (uint32_t)e;
  std::stable_sort(order.begin(), order.end(), [match_ptr](uint32_t x, uint32_t y) {
    return match_ptr[x + 1] - match_ptr[x] > match_ptr[y + 1] - match_ptr[y];
  });

  FlatLayout L;
  const auto s_ord = L.take<uint32_t>(E), s_i = L.take<uint32_t>(E), s_j = L.take<uint32_t>(E);
  const auto s_ptr = L.take<uint64_t>(E + 1); const auto s_m = L.take<double4>(M);
  const auto s_k = L.take<double>(6 * E), s_rot = L.take<double>(3 * N), s_in = L.take<double>(3 * E), s_plane = L.take<double>(3 * M),
             s_out = L.take<double>(3 * E);
  const auto s_st = L.take<int32_t>(E), s_it = L.take<int32_t>(E); const auto s_cost = L.take<double>(E);
  FlatCall fc;
  if (int st = fc.commit(L, "the translation refinement", 1)) return (gsfm_status)st;
  HIPCHK_S(fc.upload(s_ord, order.data(), E)); HIPCHK_S(fc.upload(s_i, edge_i, E)); HIPCHK_S(fc.upload(s_j, edge_j, E));
  HIPCHK_S(fc.upload(s_ptr, match_ptr, E + 1));
  if (M > 0) HIPCHK_S(fc.upload(s_m, matches, M));
  HIPCHK_S(fc.upload(s_k, intrinsics, 6 * E));
  if (N > 0) HIPCHK_S(fc.upload(s_rot, rot_aa, 3 * N));
  HIPCHK_S(fc.upload(s_in, rel_t_in, 3 * E));
  TrArgs a{};
  a.n_edges = E; a.n_matches = M;
  a.order = fc.ptr(s_ord); a.edge_i = fc.ptr(s_i); a.edge_j = fc.ptr(s_j); a.match_ptr = fc.ptr(s_ptr); a.matches = fc.ptr(s_m); a.intr = fc.ptr(s_k);
  a.rot_aa = fc.ptr(s_rot); a.rel_t_in = fc.ptr(s_in); a.plane = fc.ptr(s_plane);
  a.rel_t_out = fc.ptr(s_out); a.status = fc.ptr(s_st); a.iters = fc.ptr(s_it); a.cost = fc.ptr(s_cost);
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_tr_refine, dim3((unsigned)E), dim3(64), 0, fc.s, a);
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(rel_t_out, s_out, 3 * E));
  HIPCHK_S(fc.download(status_out, s_st, E));
  if (iters_out) HIPCHK_S(fc.download(iters_out, s_it, E));
  if (cost_out) HIPCHK_S(fc.download(cost_out, s_cost, E));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  return GSFM_OK;
}

}  // namespace
