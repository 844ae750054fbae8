// Host side of gsfm_pos_refine_relative_translations (include/gsfm_pos.h): validation, the launch order (edges by descending match
// count), one device slab and the one launch of trans_refine_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "host_common.hpp"
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

  struct Guard {
    hipStream_t s = nullptr; hipEvent_t ev[2] = {}; void* slab = nullptr;
    ~Guard() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); if (slab) (void)hipFree(slab); if (s) (void)hipStreamDestroy(s); }
  } Gd;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up(bytes); return o; };
  const size_t o_ord = take(4 * E), o_i = take(4 * E), o_j = take(4 * E), o_ptr = take(8 * (E + 1)), o_m = take(32 * M), o_k = take(48 * E),
               o_rot = take(24 * N), o_in = take(24 * E), o_plane = take(24 * M), o_out = take(24 * E), o_st = take(4 * E), o_it = take(4 * E),
               o_cost = take(8 * E), total = off;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b < (double)total * 1.02 + (64u << 20))
    return (gsfm_status)fail(GSFM_ERR_HIP, "not enough free device memory for the translation refinement (" + std::to_string((long long)(total >> 20)) +
                             " MiB needed, " + std::to_string((long long)(free_b >> 20)) + " MiB free)");
  (void)hipGetLastError();
  HIPCHK_S(hipStreamCreateWithFlags(&Gd.s, hipStreamNonBlocking));
  for (hipEvent_t& e : Gd.ev) HIPCHK_S(hipEventCreate(&e));
  if (hipMalloc(&Gd.slab, total) != hipSuccess) { Gd.slab = nullptr; (void)hipGetLastError(); return (gsfm_status)fail(GSFM_ERR_HIP, "allocating the translation refinement's buffers failed"); }
  char* base = (char*)Gd.slab;
  const hipStream_t s = Gd.s;
  HIPCHK_S(hipMemcpyAsync(base + o_ord, order.data(), 4 * E, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_i, edge_i, 4 * E, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_j, edge_j, 4 * E, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_ptr, match_ptr, 8 * (E + 1), hipMemcpyHostToDevice, s));
  if (M > 0) HIPCHK_S(hipMemcpyAsync(base + o_m, matches, 32 * M, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_k, intrinsics, 48 * E, hipMemcpyHostToDevice, s));
  if (N > 0) HIPCHK_S(hipMemcpyAsync(base + o_rot, rot_aa, 24 * N, hipMemcpyHostToDevice, s));
  HIPCHK_S(hipMemcpyAsync(base + o_in, rel_t_in, 24 * E, hipMemcpyHostToDevice, s));
  TrArgs a{};
  a.n_edges = E; a.n_matches = M;
  a.order = (const uint32_t*)(base + o_ord); a.edge_i = (const uint32_t*)(base + o_i); a.edge_j = (const uint32_t*)(base + o_j);
  a.match_ptr = (const uint64_t*)(base + o_ptr); a.matches = (const double4*)(base + o_m); a.intr = (const double*)(base + o_k);
  a.rot_aa = (const double*)(base + o_rot); a.rel_t_in = (const double*)(base + o_in); a.plane = (double*)(base + o_plane);
  a.rel_t_out = (double*)(base + o_out); a.status = (int32_t*)(base + o_st); a.iters = (int32_t*)(base + o_it); a.cost = (double*)(base + o_cost);
  HIPCHK_S(hipEventRecord(Gd.ev[0], s));
  hipLaunchKernelGGL(k_tr_refine, dim3((unsigned)E), dim3(64), 0, s, a);
  HIPCHK_S(hipEventRecord(Gd.ev[1], s));
  HIPCHK_S(hipMemcpyAsync(rel_t_out, base + o_out, 24 * E, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipMemcpyAsync(status_out, base + o_st, 4 * E, hipMemcpyDeviceToHost, s));
  if (iters_out) HIPCHK_S(hipMemcpyAsync(iters_out, base + o_it, 4 * E, hipMemcpyDeviceToHost, s));
  if (cost_out) HIPCHK_S(hipMemcpyAsync(cost_out, base + o_cost, 8 * E, hipMemcpyDeviceToHost, s));
  HIPCHK_S(hipStreamSynchronize(s));
  HIPCHK_S(hipGetLastError());
  if (kernel_ms) { float ms = 0; (void)hipEventElapsedTime(&ms, Gd.ev[0], Gd.ev[1]); *kernel_ms = ms; }
  return GSFM_OK;
}

}  // namespace
