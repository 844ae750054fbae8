// Host side of gsfm_rot_edge_sq_norms (include/gsfm_rot.h): validation, one device slab, k_cam_cache and the one sweep of k_edge_sweep.
// Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "flat_call.hpp"

namespace {

gsfm_status edge_sq_norms_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                               const double* cov6, const double* rot_aa, double max_sq_norm, double* s_out, uint8_t* keep_out,
                               uint64_t* n_kept, double* kernel_ms) {
  if (n_cams == 0 || n_edges == 0) { if (n_kept) *n_kept = 0; return GSFM_OK; }
  if (!edge_i || !edge_j || !rel_aa || !rot_aa || !s_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t e = 0; e < n_edges; ++e) if (edge_i[e] >= n_cams || edge_j[e] >= n_cams) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge with an out-of-range camera index");
  // (no host fallback: like every entry point of this library the sweep runs on the device or fails loudly)
  if (const char* why = no_device_reason("the edge sweep")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  const size_t E = n_edges, N = n_cams;
  FlatLayout L;
  const auto s_i = L.take<uint32_t>(E), s_j = L.take<uint32_t>(E);
  const auto s_rel = L.take<double>(3 * E), s_cov = L.take<double>(cov6 ? 6 * E : 0), s_rot = L.take<double>(3 * N), s_s = L.take<double>(E);
  const auto s_q = L.take<double2>(2 * N); const auto s_keep = L.take<uint8_t>(keep_out ? E : 0); const auto s_cnt = L.take<unsigned long long>(1);
  FlatCall fc;
  if (int st = fc.commit(L, "the edge sweep", 1)) return (gsfm_status)st;
  HIPCHK_S(fc.upload(s_i, edge_i, E)); HIPCHK_S(fc.upload(s_j, edge_j, E));
  HIPCHK_S(fc.upload(s_rel, rel_aa, 3 * E)); HIPCHK_S(fc.upload(s_rot, rot_aa, 3 * N));
  if (cov6) HIPCHK_S(fc.upload(s_cov, cov6, 6 * E));
  HIPCHK_S(fc.zero(s_cnt, 1));
  hipLaunchKernelGGL(k_cam_cache, dim3(grid_for(n_cams)), dim3(GSFM_BLOCK), 0, fc.s, (const double*)fc.ptr(s_rot), n_cams, 3, fc.ptr(s_q));
  EdgeSweepArgs a{};
  a.n = n_edges; a.ei = fc.ptr(s_i); a.ej = fc.ptr(s_j); a.rel_aa = fc.ptr(s_rel); a.cov6 = cov6 ? fc.ptr(s_cov) : nullptr;
  a.q = fc.ptr(s_q); a.max_sq = max_sq_norm; a.s_out = fc.ptr(s_s); a.keep = keep_out ? fc.ptr(s_keep) : nullptr; a.n_kept = fc.ptr(s_cnt);
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_edge_sweep, dim3(grid_for(n_edges)), dim3(GSFM_BLOCK), 0, fc.s, a);
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(s_out, s_s, E));
  if (keep_out) HIPCHK_S(fc.download(keep_out, s_keep, E));
  unsigned long long cnt = 0;
  HIPCHK_S(fc.download(&cnt, s_cnt, 1));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  if (n_kept) *n_kept = keep_out ? (uint64_t)cnt : n_edges;
  return GSFM_OK;
}

}  // namespace
