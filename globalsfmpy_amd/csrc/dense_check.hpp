// Host side of gsfm_rot_dense_factor_check (include/gsfm_rot.h): the exact step's Cholesky schedules on matrices the caller hands in --
// validation against the product's own limits, the assembly kernels' tiled layout built on the host, one device slab, one factorisation.
// Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "flat_call.hpp"
#include "solver_dense.hpp"
#include "solver_components.hpp"

namespace {

gsfm_status dense_factor_check_impl(int32_t schedule, uint32_t n_items, const uint32_t* n, const double* A, const double* b, const int32_t* active,
                                    double* x_out, double* L_out, int32_t* info_out) {
  if (!n || !A || !b || !x_out || !info_out || n_items == 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument or no matrix");
  if (schedule < 0 || schedule > 2) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "schedule: 0 (look2), 1 (fused) or 2 (batch)");
  if (schedule != 2 && (n_items != 1 || active)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the single schedules take one matrix and no activity flags");
  // the product's own limits: the single step up to GSFM_DENSE_MAX_T block rows (GSFM_CHOL_FUSED_MAX_T fused), a batch item up to dense_cholesky_max_cams cameras
  const uint32_t maxT = schedule == 0 ? GSFM_DENSE_MAX_T : schedule == 1 ? GSFM_CHOL_FUSED_MAX_T : 0;
  const uint64_t max_n = schedule == 2 ? 3 * (uint64_t)std::max(default_options().dense_cholesky_max_cams, 0) : (uint64_t)maxT * GSFM_CB;
  for (uint32_t i = 0; i < n_items; ++i) {
    if (n[i] == 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "a matrix with no unknowns");
    if (n[i] > max_n) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "matrix beyond the size the exact step supports on this schedule");
  }
  if (const char* why = no_device_reason("the dense factorisation check")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  // host side of the assembly kernels' layout (k_dense_assemble, k_comp_assemble): the lower triangle in tiles, identity on the padding
  // diagonal n .. 32 T - 1, the right-hand side in the first row of block row T; then one slab: A of all items, L, x, info, activity, items
  std::vector<uint32_t> T(n_items);
  std::vector<size_t> offA(n_items), offL(n_items), offX(n_items), offIn(n_items);
  size_t words = 0, in_words = 0;
  uint32_t Tmax = 0;
  for (uint32_t i = 0; i < n_items; ++i) { T[i] = (n[i] + GSFM_CB - 1) / GSFM_CB; Tmax = std::max(Tmax, T[i]); offA[i] = words; words += chol_num_tiles(T[i]) * GSFM_TILE_ELEMS; offIn[i] = in_words; in_words += (size_t)n[i] * n[i]; }
  const size_t a_words = words;
  for (uint32_t i = 0; i < n_items; ++i) { offL[i] = words; words += chol_num_tiles(T[i]) * GSFM_TILE_ELEMS; }
  for (uint32_t i = 0; i < n_items; ++i) { offX[i] = words; words += (size_t)T[i] * GSFM_CB; }
  std::vector<double> hA;
  try { hA.assign(a_words, 0.0); } catch (const std::exception&) { return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "out of host memory"); }
  size_t b_off = 0;
  for (uint32_t i = 0; i < n_items; ++i) {
    double* At = hA.data() + offA[i];
    const double* Ai = A + offIn[i];
    auto elem = [&](uint32_t g, uint32_t h) -> double& { return At[chol_tile_off(g / GSFM_CB, h / GSFM_CB) + (g % GSFM_CB) * GSFM_CB + h % GSFM_CB]; };
    for (uint32_t g = 0; g < n[i]; ++g) for (uint32_t h = 0; h <= g; ++h) elem(g, h) = Ai[(size_t)g * n[i] + h];
    for (uint32_t g = n[i]; g < T[i] * GSFM_CB; ++g) elem(g, g) = 1.0;
    for (uint32_t g = 0; g < n[i]; ++g) At[chol_tile_off(T[i], g / GSFM_CB) + g % GSFM_CB] = b[b_off + g];
    b_off += n[i];
  }
  FlatLayout L;
  const auto s_w = L.take<double>(words); const auto s_info = L.take<int>(n_items), s_act = L.take<int>(n_items); const auto s_items = L.take<CholBatchItem>(n_items);
  FlatCall fc;
  if (int st = fc.commit(L, "the dense factorisation check", 0)) return (gsfm_status)st;
  double* dw = fc.ptr(s_w); int* dinfo = fc.ptr(s_info); int* dact = fc.ptr(s_act);
  HIPCHK_S(hipMemsetAsync(fc.slab, 0, L.total, fc.s));
  HIPCHK_S(fc.upload(s_w, hA.data(), a_words));
  if (schedule == 2) {
    std::vector<int> act(n_items, 1);
    if (active) for (uint32_t i = 0; i < n_items; ++i) act[i] = active[i] != 0;
    std::vector<CholBatchItem> items(n_items);
    for (uint32_t i = 0; i < n_items; ++i) items[i] = CholBatchItem{dw + offA[i], dw + offL[i], dw + offX[i], T[i], n[i], dinfo + i, dact + i};
    HIPCHK_S(fc.upload(s_act, act.data(), n_items));
    HIPCHK_S(fc.upload(s_items, items.data(), n_items));
    HIPCHK_S(hipStreamSynchronize(fc.s));   // (the staging vectors die with this scope)
    enqueue_chol_batch(fc.ptr(s_items), n_items, Tmax, fc.s, false);
  } else {
    enqueue_chol_solve(dw + offA[0], dw + offL[0], dw + offX[0], n[0], T[0], dinfo, fc.s, schedule == 1);
  }
  HIPCHK_S(hipGetLastError());
  std::vector<double> hw(words - a_words);
  std::vector<int> hinfo(n_items);
  HIPCHK_S(hipMemcpyAsync(hw.data(), dw + a_words, sizeof(double) * hw.size(), hipMemcpyDeviceToHost, fc.s));   // (L and x: the slot's tail)
  HIPCHK_S(fc.download(hinfo.data(), s_info, n_items));
  HIPCHK_S(fc.sync());
  size_t x_off = 0, l_off = 0;
  for (uint32_t i = 0; i < n_items; ++i) {
    info_out[i] = hinfo[i];
    const double* Lt = hw.data() + (offL[i] - a_words);
    const double* xt = hw.data() + (offX[i] - a_words);
    for (uint32_t g = 0; g < n[i]; ++g) x_out[x_off + g] = xt[g];
    x_off += n[i];
    if (L_out) {
      double* Li = L_out + l_off;
      for (uint32_t g = 0; g < n[i]; ++g) for (uint32_t h = 0; h < n[i]; ++h)
        Li[(size_t)g * n[i] + h] = h <= g ? Lt[chol_tile_off(g / GSFM_CB, h / GSFM_CB) + (g % GSFM_CB) * GSFM_CB + h % GSFM_CB] : 0.0;
      l_off += (size_t)n[i] * n[i];
    }
  }
  return GSFM_OK;
}

}  // namespace
