// Host side of gsfm_pos_filter_relative_translations (include/gsfm_pos.h): validation, the per-camera CSR, the axes' generator, one
// device slab (flat_call.hpp) and the launch sequence of trans_filter_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "flat_call.hpp"
#include "spanning_tree.hpp"
#include "trans_filter_kernels.hpp"
#include "../../include/gsfm_pos.h"

namespace {

// The library's own standard normals (the axes of the filter): splitmix64 -> two uniforms in (0, 1) -> Box-Muller's cosine branch.
struct TfNormals {
  uint64_t s;
  explicit TfNormals(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uniform() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal() { const double u1 = uniform(), u2 = uniform(); return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925 * u2); }
};

// axis_k = normalise(mean + var o z_k)  (the reference hands the variance to a parameter named std_dev; kept)
void tf_generate_axes(const double* stats, int32_t n_axes, uint64_t seed, double* axes) {
  TfNormals rng(seed);
  for (int32_t k = 0; k < n_axes; ++k) {
    double v[3];
    for (int c = 0; c < 3; ++c) v[c] = stats[c] + stats[3 + c] * rng.normal();
    const double nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (nrm > 0.0 && std::isfinite(nrm)) { for (int c = 0; c < 3; ++c) axes[3 * k + c] = v[c] / nrm; }
    else { axes[3 * k] = 1.0; axes[3 * k + 1] = 0.0; axes[3 * k + 2] = 0.0; }   // (a zero or non-finite draw: the x axis)
  }
}

gsfm_status trans_filter_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                              const double* rot_aa, int32_t n_axes, const double* axes, uint64_t seed, double tolerance, double* bad_weight_out,
                              uint8_t* keep_out, uint64_t* n_kept, double* stats_out, double* axes_out, double* proj_out, uint32_t* num_passes_out,
                              uint32_t* num_picks_out, double* kernel_ms) {
  if (n_axes < 1 || n_axes > 65535) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the translation filter takes 1 to 65535 projections");
  if (!edge_i || !edge_j || !rel_t || !rot_aa || !bad_weight_out || !keep_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31) || n_cams >= (1u << 31)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges or cameras)");
  const int64_t bad = first_bad_edge(n_cams, n_edges, edge_i, edge_j);
  if (bad >= 0)
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(bad) + " has an out-of-range camera index or joins a camera to itself");
  if (n_kept) *n_kept = 0;
  if (n_edges == 0 || n_cams == 0) return GSFM_OK;   // nothing to filter
  const size_t N = n_cams, E = n_edges, ND = 2 * E, A = (size_t)n_axes, G = (N + GSFM_TF_GROUP - 1) / GSFM_TF_GROUP;
  // the integer sums of a camera must stay below 2^63: |p| <= |t| |axis|, q <= |p| 2^32 + 1
  double axis_norm = 1.0;
  if (axes)
    for (size_t k = 0; k < A; ++k) axis_norm = std::fmax(axis_norm, std::sqrt(axes[3 * k] * axes[3 * k] + axes[3 * k + 1] * axes[3 * k + 1] + axes[3 * k + 2] * axes[3 * k + 2]));
  if (!std::isfinite(axis_norm)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "a non-finite projection axis");
  {
    std::vector<double> load(N, 0.0);
    for (size_t e = 0; e < E; ++e) {
      const double* t = rel_t + 3 * e;
      const double w = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) * axis_norm * 1.000001 * 4294967296.0 + 1.0;
      load[edge_i[e]] += w; load[edge_j[e]] += w;
    }
    for (size_t v = 0; v < N; ++v)
      if (!(load[v] < 4611686018427387904.0))
        return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "camera " + std::to_string(v) + ": the integer arc weights could overflow 63 bits (or a translation is not finite)");
  }
  if (const char* why = no_device_reason("the translation filter")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  // per-camera CSR of directed entries, as the position problem builds it: a counting sort by neighbour, then a stable one by row
  std::vector<uint32_t> row_ptr(N + 1, 0);
  for (size_t e = 0; e < E; ++e) { row_ptr[edge_i[e] + 1]++; row_ptr[edge_j[e] + 1]++; }
  for (size_t v = 0; v < N; ++v) row_ptr[v + 1] += row_ptr[v];
  hvec<uint32_t> nbr(ND), ent(ND);
  {
    std::vector<uint32_t> by_nbr(ND), pos(row_ptr.begin(), row_ptr.end() - 1);
    for (size_t e = 0; e < E; ++e) { by_nbr[pos[edge_j[e]]++] = (uint32_t)(2 * e); by_nbr[pos[edge_i[e]]++] = (uint32_t)(2 * e + 1); }
    pos.assign(row_ptr.begin(), row_ptr.end() - 1);
    for (size_t t = 0; t < ND; ++t) {
      const uint32_t u = by_nbr[t], e = u >> 1, side = u & 1;
      const uint32_t d = pos[side ? edge_j[e] : edge_i[e]]++;
      nbr[d] = side ? edge_i[e] : edge_j[e]; ent[d] = u;
    }
  }

  // LDS while the 28 B per camera (and the group maxima) fit one workgroup's share, global memory beyond
  int dev = 0; hipDeviceProp_t prop;
  HIPCHK_S(hipGetDevice(&dev));
  HIPCHK_S(hipGetDeviceProperties(&prop, dev));
  const size_t lds_need = tf_lds_bytes(n_cams) + 512;   // + the kernel's static LDS
  bool use_lds = lds_need <= (size_t)prop.sharedMemPerBlock;
  if (use_lds && lds_need > 48 * 1024 &&
      hipFuncSetAttribute((const void*)k_tf_order<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tf_lds_bytes(n_cams)) != hipSuccess) {
    (void)hipGetLastError();
    use_lds = false;   // (the same kernel on global-memory state: the same result)
  }
  FlatLayout L;
  const auto s_i = L.take<uint32_t>(E), s_j = L.take<uint32_t>(E);
  const auto s_rel = L.take<double>(3 * E), s_rot = L.take<double>(3 * N), s_dir = L.take<double>(3 * E);
  const auto s_ptr = L.take<uint32_t>(N + 1), s_nbr = L.take<uint32_t>(ND), s_ent = L.take<uint32_t>(ND);
  const auto s_part = L.take<double>(3 * GSFM_TF_PARTS), s_stats = L.take<double>(6), s_axes = L.take<double>(3 * A);
  const auto s_pass = L.take<uint32_t>(A * N), s_cnt = L.take<uint32_t>(2 * A); const auto s_bad = L.take<double>(E); const auto s_keep = L.take<uint8_t>(E);
  const auto s_kept = L.take<unsigned long long>(1); const auto s_proj = L.take<double>(proj_out ? E * A : 0);
  const auto s_gq = L.take<unsigned long long>(use_lds ? 0 : 2 * A * N); const auto s_gmax = L.take<double>(use_lds ? 0 : A * G);
  const auto s_gu = L.take<uint32_t>(use_lds ? 0 : A * (2 * N + 2 * G));
  FlatCall fc;
  if (int st = fc.commit(L, "the translation filter", 2)) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  HIPCHK_S(fc.upload(s_i, edge_i, E)); HIPCHK_S(fc.upload(s_j, edge_j, E));
  HIPCHK_S(fc.upload(s_rel, rel_t, 3 * E)); HIPCHK_S(fc.upload(s_rot, rot_aa, 3 * N));
  HIPCHK_S(fc.upload(s_ptr, row_ptr.data(), N + 1)); HIPCHK_S(fc.upload(s_nbr, nbr.data(), ND)); HIPCHK_S(fc.upload(s_ent, ent.data(), ND));
  HIPCHK_S(fc.zero(s_kept, 1));
  const uint32_t* d_i = fc.ptr(s_i); const uint32_t* d_j = fc.ptr(s_j);
  double* d_dir = fc.ptr(s_dir); double* d_part = fc.ptr(s_part); double* d_stats = fc.ptr(s_stats); double* d_axes = fc.ptr(s_axes);
  const dim3 blk(256), gE((unsigned)((E + 255) / 256));

  // ---- directions, mean, variance ---------------------------------------------------------------------------------------------------
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_tf_directions, gE, blk, 0, s, (uint32_t)E, d_i, (const double*)fc.ptr(s_rot), (const double*)fc.ptr(s_rel), d_dir);
  hipLaunchKernelGGL(k_tf_moment, dim3(GSFM_TF_PARTS), blk, 0, s, (const double*)d_dir, (uint32_t)E, (const double*)nullptr, 0, d_part);
  hipLaunchKernelGGL(k_tf_moment_final, dim3(1), blk, 0, s, (const double*)d_part, (double)E, d_stats);
  hipLaunchKernelGGL(k_tf_moment, dim3(GSFM_TF_PARTS), blk, 0, s, (const double*)d_dir, (uint32_t)E, (const double*)d_stats, 1, d_part);
  hipLaunchKernelGGL(k_tf_moment_final, dim3(1), blk, 0, s, (const double*)d_part, (double)E - 1.0, d_stats + 3);
  HIPCHK_S(fc.end_span());
  double stats[6] = {0, 0, 0, 0, 0, 0};
  std::vector<double> h_axes(3 * A);
  if (axes) std::memcpy(h_axes.data(), axes, 24 * A);
  if (!axes || stats_out) {
    HIPCHK_S(fc.download(stats, s_stats, 6));
    HIPCHK_S(fc.sync());
    if (!axes) tf_generate_axes(stats, n_axes, seed, h_axes.data());
  }
  HIPCHK_S(fc.upload(s_axes, h_axes.data(), 3 * A));

  // ---- projections (on request), the orderings, the bad weights ------------------------------------------------------------------------
  TfOrderArgs a{};
  a.n_cams = n_cams; a.n_groups = (uint32_t)G;
  a.row_ptr = fc.ptr(s_ptr); a.nbr = fc.ptr(s_nbr); a.ent = fc.ptr(s_ent);
  a.dir_e = d_dir; a.axes = d_axes; a.pass_out = fc.ptr(s_pass); a.counts = fc.ptr(s_cnt);
  if (!use_lds) { a.g_q = fc.ptr(s_gq); a.g_gmax = fc.ptr(s_gmax); a.g_u32 = fc.ptr(s_gu); }
  HIPCHK_S(fc.begin_span());
  if (proj_out) hipLaunchKernelGGL(k_tf_proj, gE, blk, 0, s, (uint32_t)E, (const double*)d_dir, (const double*)d_axes, (int)n_axes, fc.ptr(s_proj));
  if (use_lds) hipLaunchKernelGGL(k_tf_order<true>, dim3((unsigned)A), dim3(256), tf_lds_bytes(n_cams), s, a);
  else hipLaunchKernelGGL(k_tf_order<false>, dim3((unsigned)A), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(k_tf_bad, gE, blk, 0, s, (uint32_t)E, n_cams, d_i, d_j, (const double*)d_dir, (const double*)d_axes, (int)n_axes,
                     (const uint32_t*)fc.ptr(s_pass), tolerance * (double)n_axes, fc.ptr(s_bad), fc.ptr(s_keep), fc.ptr(s_kept));
  HIPCHK_S(fc.end_span());
  std::vector<uint32_t> counts(2 * A);
  unsigned long long kept = 0;
  HIPCHK_S(fc.download(bad_weight_out, s_bad, E));
  HIPCHK_S(fc.download(keep_out, s_keep, E));
  HIPCHK_S(fc.download(&kept, s_kept, 1));
  HIPCHK_S(fc.download(counts.data(), s_cnt, 2 * A));
  if (proj_out) HIPCHK_S(fc.download(proj_out, s_proj, E * A));
  HIPCHK_S(fc.sync());
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  if (n_kept) *n_kept = kept;
  if (stats_out) std::memcpy(stats_out, stats, 48);
  if (axes_out) std::memcpy(axes_out, h_axes.data(), 24 * A);
  for (size_t k = 0; k < A; ++k) {
    if (num_passes_out) num_passes_out[k] = counts[2 * k];
    if (num_picks_out) num_picks_out[k] = counts[2 * k + 1];
  }
  return GSFM_OK;
}

}  // namespace
