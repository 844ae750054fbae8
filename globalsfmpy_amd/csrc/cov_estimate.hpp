// Host side of gsfm_cov_estimate (include/gsfm_rot.h): validation, one device slab and the one launch of cov_kernels.hpp (one wavefront
// per edge).  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "flat_call.hpp"

namespace {

gsfm_status cov_estimate_impl(uint64_t n_edges, const uint64_t* match_ptr, const double* matches, const double* intrinsics, const double* rot_in,
                              const double* trans_in, int32_t max_iterations, double* cov9_out, double* rot_out, double* trans_out,
                              int32_t* status_out, int32_t* iters_out, double* kernel_ms) {
  if (!match_ptr || !matches || !intrinsics || !rot_in || !trans_in || !cov9_out || !rot_out || !trans_out || !status_out)
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges == 0) return GSFM_OK;
  if (const char* why = no_device_reason("the covariance estimator")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  const size_t E = n_edges, M = match_ptr[n_edges];
  for (size_t e = 0; e < E; ++e) if (match_ptr[e + 1] < match_ptr[e]) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "match_ptr must be non-decreasing");
  FlatLayout L;
  const auto s_ptr = L.take<uint64_t>(E + 1); const auto s_m = L.take<double4>(M);
  const auto s_k = L.take<double>(6 * E), s_r = L.take<double>(3 * E), s_t = L.take<double>(3 * E), s_cov = L.take<double>(9 * E), s_ro = L.take<double>(3 * E),
             s_to = L.take<double>(3 * E);
  const auto s_st = L.take<int>(E), s_it = L.take<int>(E);
  FlatCall fc;
  if (int st = fc.commit(L, "the covariance estimator", 1)) return (gsfm_status)st;
  HIPCHK_S(fc.upload(s_ptr, match_ptr, E + 1));
  if (M) HIPCHK_S(fc.upload(s_m, matches, M));
  HIPCHK_S(fc.upload(s_k, intrinsics, 6 * E)); HIPCHK_S(fc.upload(s_r, rot_in, 3 * E)); HIPCHK_S(fc.upload(s_t, trans_in, 3 * E));
  CovArgs a{};
  a.n_edges = n_edges; a.match_ptr = fc.ptr(s_ptr); a.matches = fc.ptr(s_m); a.intr = fc.ptr(s_k); a.rot_in = fc.ptr(s_r); a.trans_in = fc.ptr(s_t);
  a.max_iterations = max_iterations; a.cov9 = fc.ptr(s_cov); a.rot_out = fc.ptr(s_ro); a.trans_out = fc.ptr(s_to); a.status = fc.ptr(s_st); a.iters = fc.ptr(s_it);
  const int grid = (int)((n_edges + (GSFM_BLOCK / 64) - 1) / (GSFM_BLOCK / 64));
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_cov_estimate, dim3(grid), dim3(GSFM_BLOCK), 0, fc.s, a);
  HIPCHK_S(fc.end_span());
  HIPCHK_S(fc.download(cov9_out, s_cov, 9 * E)); HIPCHK_S(fc.download(rot_out, s_ro, 3 * E)); HIPCHK_S(fc.download(trans_out, s_to, 3 * E));
  HIPCHK_S(fc.download(status_out, s_st, E));
  if (iters_out) HIPCHK_S(fc.download(iters_out, s_it, E));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  return GSFM_OK;
}

}  // namespace
