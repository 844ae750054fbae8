// gsfm_tracks_select_good and gsfm_tracks_select_good_from_statistics (include/gsfm_tracks.h): Theia's SelectGoodTracksForBundleAdjustment.
// Plain C++ first (no HIP: a host compiler alone builds it, as it builds the first half of track_build.hpp): the argument checks, the cell of a
// coordinate, step 2 as sequential code, and the walk of step 3 both entries share -- the device entry replays it over the items of the
// deficient cameras it downloads, the host entry over all items.  Under hipcc: the host side of the device call on the scene and launcher of
// track_scene.hpp, launching track_select_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "track_scene.hpp"

namespace {

struct TsParams { uint32_t L = 10, K = 200; int32_t S = 100; int capacity_log2 = 0; double inv = 0.01; };
constexpr uint64_t TS_NAN_BITS = 0x7ff8000000000000ull;

// the smallest capacity the cell table may have, and the one it gets by default (log2)
inline int ts_min_capacity_log2(uint64_t n_items) { int k = 0; while ((1ull << k) < n_items) ++k; return k; }
inline int ts_auto_capacity_log2(uint64_t n_items) { return std::max(10, ts_min_capacity_log2(2 * n_items)); }

inline bool ts_params_ok(int32_t L, int32_t S, int32_t K, int32_t capacity_log2, TsParams* p, std::string* why) {
  auto refuse = [why](const std::string& message) { *why = message; return false; };
  if (L < 1) return refuse("long_track_length_threshold must be at least 1");
  if (S < 1) return refuse("image_grid_cell_size_pixels must be at least 1");
  if (K < 0) return refuse("min_num_optimized_tracks_per_view must not be negative");
  if (capacity_log2 < 0 || capacity_log2 > 31) return refuse("hash_capacity_log2 must be 0 (automatic) or at most 31");
  p->L = (uint32_t)L; p->S = S; p->K = (uint32_t)K; p->capacity_log2 = capacity_log2; p->inv = 1.0 / (double)S;
  return true;
}
// every coordinate finite and its cell inside the int32 range (after track_obs_ok)
inline bool ts_coordinates_ok(uint64_t n_obs, const double* obs_xy, double inv, std::string* why) {
  for (uint64_t k = 0; k < 2 * n_obs; ++k) {
    if (!std::isfinite(obs_xy[k])) { *why = "observation " + std::to_string(k / 2) + " has a coordinate that is not finite"; return false; }
    if (!(std::fabs(obs_xy[k] * inv) < 2147483648.0)) { *why = "observation " + std::to_string(k / 2) + " lies outside the grid (|x / cell size| >= 2^31)"; return false; }
  }
  return true;
}
inline int32_t ts_cell(double x, double inv) { return (int32_t)(x * inv); }   // one multiplication, truncation toward zero
inline uint64_t ts_mean_bits(double m) { if (m != m) return TS_NAN_BITS; uint64_t b; std::memcpy(&b, &m, 8); return b; }

struct TsItem {   // an item as step 3 walks it
  uint32_t cam, track, place;
  bool operator<(const TsItem& o) const { return cam != o.cam ? cam < o.cam : track != o.track ? track < o.track : place < o.place; }
};

// Step 3 over items sorted by (camera, track, place); every item of a camera that occurs is in the list.  selected: 0 / 1 / 2 per track, updated.
inline void ts_top_up(const TsItem* items, size_t n, uint32_t K, uint8_t* selected, uint64_t* n_cameras, uint64_t* n_tracks_added) {
  *n_cameras = 0; *n_tracks_added = 0;
  if (K == 0) return;
  std::vector<size_t> take;
  for (size_t i = 0, j; i < n; i = j) {
    for (j = i; j < n && items[j].cam == items[i].cam; ++j) {}
    const uint64_t est = j - i;
    uint64_t opt = 0;
    for (size_t k = i; k < j; ++k) opt += selected[items[k].track] != 0;
    if (opt >= K || opt == est) continue;
    const uint64_t m = std::min<uint64_t>(K - opt, est - opt);
    take.clear();   // the first m items whose track is not selected as the camera's turn begins
    for (size_t k = i; k < j && take.size() < m; ++k) if (!selected[items[k].track]) take.push_back(k);
    for (size_t k : take) if (!selected[items[k].track]) { selected[items[k].track] = 2; ++*n_tracks_added; }
    ++*n_cameras;
  }
}

struct TsCellKey {
  uint32_t cam; int32_t cx, cy;
  bool operator==(const TsCellKey& k) const { return cam == k.cam && cx == k.cx && cy == k.cy; }
};
struct TsCellHash {
  size_t operator()(const TsCellKey& k) const {
    uint64_t h = ((uint64_t)(uint32_t)k.cx << 32 | (uint32_t)k.cy) * 0x9e3779b97f4a7c15ull; h ^= h >> 29; h += k.cam; h *= 0xbf58476d1ce4e5b9ull;
    return (size_t)(h ^ (h >> 32));
  }
};
struct TsBest { uint32_t len; uint64_t mean; uint32_t track; };

// Steps 2 and 3 sequentially, given the statistics (arguments checked by the caller; selected_out is all 0 on entry)
inline void ts_sequential(uint32_t n_cams, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                          const uint8_t* point_estimated, const int32_t* n_views, const double* mean_sq_err, const TsParams& p, uint8_t* selected_out, uint64_t counts[6]) {
  std::unordered_map<TsCellKey, TsBest, TsCellHash> cells;
  std::vector<uint64_t> cam_begin((size_t)n_cams + 1, 0);
  uint64_t n_items = 0;
  auto for_items = [&](auto fn) {
    for (uint64_t t = 0; t < n_tracks; ++t) {
      if (point_estimated && !point_estimated[t]) continue;
      for (uint64_t o = track_ptr[t]; o < track_ptr[t + 1]; ++o)
        if (!cam_estimated || cam_estimated[obs_cam[o]]) fn((uint32_t)t, o);
    }
  };
  for (uint64_t t = 0; t < n_tracks; ++t) counts[0] += (!point_estimated || point_estimated[t]) && n_views[t] >= 1;
  for_items([&](uint32_t t, uint64_t o) {
    ++cam_begin[obs_cam[o] + 1]; ++n_items;
    const TsBest mine{std::min((uint32_t)n_views[t], p.L), ts_mean_bits(mean_sq_err[t]), t};
    const auto it = cells.emplace(TsCellKey{obs_cam[o], ts_cell(obs_xy[2 * o], p.inv), ts_cell(obs_xy[2 * o + 1], p.inv)}, mine);
    TsBest& b = it.first->second;
    if (mine.len != b.len ? mine.len < b.len : mine.mean != b.mean ? mine.mean < b.mean : mine.track < b.track) b = mine;
  });
  counts[1] = cells.size();
  for (const auto& c : cells) selected_out[c.second.track] = 1;
  for (uint64_t t = 0; t < n_tracks; ++t) counts[2] += selected_out[t] == 1;
  // all items by (camera, track, place): a counting sort by camera keeps the walk's (track, place) order
  for (uint32_t c = 0; c < n_cams; ++c) cam_begin[c + 1] += cam_begin[c];
  std::vector<TsItem> items((size_t)n_items);
  for_items([&](uint32_t t, uint64_t o) { items[(size_t)cam_begin[obs_cam[o]]++] = TsItem{obs_cam[o], t, (uint32_t)(o - track_ptr[t])}; });
  ts_top_up(items.data(), items.size(), p.K, selected_out, &counts[3], &counts[4]);
  counts[5] = counts[2] + counts[4];
}

// The checks both entries share, in the order they report them, after the parameters: the track arrays, then the coordinates
inline bool ts_arrays_ok(uint32_t n_cams, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, double inv, std::string* why) {
  if (!track_ptr_ok(n_tracks, track_ptr, TrackLimit::tracks_and_lengths, 0, true, "NULL argument", why)) return false;
  if (track_ptr[n_tracks] >= (1ull << 31)) { *why = "problem too large (2^31 observations)"; return false; }   // (before any observation is read)
  if (!track_obs_ok(n_cams, track_ptr[n_tracks], obs_cam, obs_xy, why)) return false;
  return ts_coordinates_ok(track_ptr[n_tracks], obs_xy, inv, why);
}

}  // namespace

#ifdef __HIPCC__
#include "track_select_kernels.hpp"

namespace {

gsfm_status select_good_from_statistics_impl(uint32_t n_cams, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                             const double* obs_xy, const uint8_t* point_estimated, const int32_t* n_views, const double* mean_sq_err,
                                             int32_t long_track_length_threshold, int32_t image_grid_cell_size_pixels, int32_t min_num_optimized_tracks_per_view,
                                             uint8_t* selected_out, uint64_t* counts_out) {
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  TsParams p;
  std::string why;
  if (!ts_params_ok(long_track_length_threshold, image_grid_cell_size_pixels, min_num_optimized_tracks_per_view, 0, &p, &why)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
  if (n_tracks == 0) return GSFM_OK;
  if (!selected_out || !n_views || !mean_sq_err) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!ts_arrays_ok(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, p.inv, &why)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
  for (uint64_t t = 0; t < n_tracks; ++t)
    if ((!point_estimated || point_estimated[t]) && n_views[t] < 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "track " + std::to_string(t) + " has a negative n_views");
  std::memset(selected_out, 0, n_tracks);
  ts_sequential(n_cams, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy, point_estimated, n_views, mean_sq_err, p, selected_out, counts);
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  return GSFM_OK;
}

gsfm_status select_good_impl(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks,
                             const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const double* points, const uint8_t* point_estimated,
                             int32_t long_track_length_threshold, int32_t image_grid_cell_size_pixels, int32_t min_num_optimized_tracks_per_view,
                             int32_t hash_capacity_log2, uint8_t* selected_out, int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms,
                             double* top_up_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (top_up_out) top_up_out[0] = top_up_out[1] = 0.0;
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  TsParams p;
  std::string why;
  if (!ts_params_ok(long_track_length_threshold, image_grid_cell_size_pixels, min_num_optimized_tracks_per_view, hash_capacity_log2, &p, &why))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
  if (n_tracks == 0) return GSFM_OK;   // nothing to select from
  if (!points || !selected_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_cams > 0 && (!rot_aa || !cam_pos || !intrinsics)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!ts_arrays_ok(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, p.inv, &why)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);

  const size_t T = n_tracks, O = track_ptr[T], N = n_cams;
  uint64_t n_items = 0;
  for (size_t t = 0; t < T; ++t) {
    if (point_estimated && !point_estimated[t]) continue;
    for (uint64_t o = track_ptr[t]; o < track_ptr[t + 1]; ++o) n_items += !cam_estimated || cam_estimated[obs_cam[o]];
  }
  if (p.capacity_log2 != 0 && p.capacity_log2 < ts_min_capacity_log2(n_items))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "hash_capacity_log2 = " + std::to_string(p.capacity_log2) + " gives fewer slots than the " + std::to_string(n_items) + " items");
  std::memset(selected_out, 0, T);
  if (n_views_out) std::memset(n_views_out, 0, T * sizeof(int32_t));
  if (mean_sq_err_out) std::memset(mean_sq_err_out, 0, T * sizeof(double));

  // the launch order of the outlier rule: the tracks that are not estimated never reach the device
  hvec<uint32_t> order(T);
  uint64_t all[4], cb[4];
  tri_bucket(T, track_ptr, order.data(), all);
  const size_t E = tri_keep_estimated(order.data(), all, point_estimated, cb);
  if (E == 0) return GSFM_OK;   // no track is estimated: nothing for the device
  if (const char* reason = no_device_reason("the track selection")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, reason);

  const int cap_log2 = p.capacity_log2 ? p.capacity_log2 : ts_auto_capacity_log2(n_items);
  const size_t capacity = (size_t)1 << cap_log2;
  FlatLayout L;
  TrackScene sc;
  sc.take(L, E, T, N, O, false);   // (no ray store: the plane of the 64-lane class is not taken)
  const auto s_item = L.take<uint32_t>(O), s_slot = L.take<uint32_t>(O), s_table = L.take<uint32_t>(capacity), s_clen = L.take<uint32_t>(capacity);
  const auto s_cmean = L.take<unsigned long long>(capacity);
  const auto s_ctrack = L.take<uint32_t>(capacity), s_est = L.take<uint32_t>(N), s_opt = L.take<uint32_t>(N), s_list = L.take<uint32_t>(3 * O), s_cnt = L.take<uint32_t>(TS_N_COUNTERS);
  const auto s_sel = L.take<uint8_t>(T);
  FlatCall fc;
  if (int st = fc.commit(L, "the track selection", 1)) return (gsfm_status)st;
  if (int st = sc.upload(fc, order.data(), track_ptr, obs_cam, obs_xy, rot_aa, cam_pos, intrinsics, cam_estimated)) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  HIPCHK_S(fc.upload(sc.s_pt, points, 3 * T));
  HIPCHK_S(fc.zero(sc.s_nv, T)); HIPCHK_S(fc.zero(sc.s_err, T)); HIPCHK_S(fc.zero(s_sel, T)); HIPCHK_S(fc.zero(s_cnt, (size_t)TS_N_COUNTERS));
  if (N > 0) { HIPCHK_S(fc.zero(s_est, N)); HIPCHK_S(fc.zero(s_opt, N)); }
  if (O > 0) HIPCHK_S(hipMemsetAsync(fc.ptr(s_item), 0xff, 4 * O, s));   // GSFM_TS_NONE where k_track_stats does not write
  HIPCHK_S(hipMemsetAsync(fc.ptr(s_table), 0xff, 4 * capacity, s)); HIPCHK_S(hipMemsetAsync(fc.ptr(s_clen), 0xff, 4 * capacity, s));
  HIPCHK_S(hipMemsetAsync(fc.ptr(s_cmean), 0xff, 8 * capacity, s)); HIPCHK_S(hipMemsetAsync(fc.ptr(s_ctrack), 0xff, 4 * capacity, s));

  TriArgs a{};
  HIPCHK_S(fc.begin_span());
  sc.start(fc, cam_estimated != nullptr, 0.0, 0.0, &a);   // (neither bound is read: the statistics kernel gates nothing)
  a.point = nullptr; a.plane = nullptr;
  for_lane_classes(cb, [&](auto G, uint64_t n_slots, uint64_t offset, dim3 grid, dim3 block) {
    a.n_slots = n_slots; a.order = fc.ptr(sc.s_ord) + offset;
    hipLaunchKernelGGL(k_track_stats<G()>, grid, block, 0, s, a, (const double*)fc.ptr(sc.s_pt), fc.ptr(s_item));
  });
  TsArgs ts{};
  ts.n_obs = (uint32_t)O; ts.obs_cam = fc.ptr(sc.s_cam); ts.obs_xy = fc.ptr(sc.s_xy); ts.track_ptr = (const unsigned long long*)fc.ptr(sc.s_ptr);
  ts.item_track = fc.ptr(s_item); ts.n_views = fc.ptr(sc.s_nv); ts.mean_sq_err = fc.ptr(sc.s_err); ts.inv_cell = p.inv; ts.long_len = p.L;
  ts.mask = (uint32_t)(capacity - 1); ts.table = fc.ptr(s_table); ts.slot_of = fc.ptr(s_slot); ts.cell_len = fc.ptr(s_clen); ts.cell_mean = fc.ptr(s_cmean);
  ts.cell_track = fc.ptr(s_ctrack); ts.selected = fc.ptr(s_sel); ts.cam_est = fc.ptr(s_est); ts.cam_opt = fc.ptr(s_opt); ts.min_per_view = p.K;
  ts.list = fc.ptr(s_list); ts.counters = fc.ptr(s_cnt);
  if (n_items > 0) {
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((O + 255) / 256, 16384))), blk(256);
    hipLaunchKernelGGL(k_ts_insert, grid, blk, 0, s, ts);
    hipLaunchKernelGGL(k_ts_mean, grid, blk, 0, s, ts);
    hipLaunchKernelGGL(k_ts_track, grid, blk, 0, s, ts);
    hipLaunchKernelGGL(k_ts_mark, grid, blk, 0, s, ts);
    hipLaunchKernelGGL(k_ts_count, grid, blk, 0, s, ts);
    if (p.K > 0) hipLaunchKernelGGL(k_ts_deficient, grid, blk, 0, s, ts);
  }
  HIPCHK_S(fc.end_span());
  uint32_t h_cnt[TS_N_COUNTERS];
  hvec<int32_t> nv(T);
  HIPCHK_S(fc.download(h_cnt, s_cnt, (size_t)TS_N_COUNTERS));
  HIPCHK_S(fc.download(selected_out, s_sel, T));
  HIPCHK_S(fc.download(nv.data(), sc.s_nv, T));
  if (mean_sq_err_out) HIPCHK_S(fc.download(mean_sq_err_out, sc.s_err, T));
  HIPCHK_S(fc.sync());
  if (h_cnt[TS_ERR]) return (gsfm_status)fail(GSFM_ERR_HIP, "the track selection's cell table overflowed");
  const size_t n_list = h_cnt[TS_LIST];
  if (n_list > O) return (gsfm_status)fail(GSFM_ERR_HIP, "the track selection's list of deficient items is longer than the observations");
  hvec<TsItem> items(n_list);
  static_assert(sizeof(TsItem) == 12, "the device writes three 32-bit words per item");
  if (n_list > 0) { HIPCHK_S(fc.download((uint32_t*)items.data(), s_list, 3 * n_list)); HIPCHK_S(fc.sync()); }
  for (const TsItem& it : items) if (it.cam >= N || it.track >= T) return (gsfm_status)fail(GSFM_ERR_HIP, "the track selection's list of deficient items is damaged");
  if (kernel_ms) *kernel_ms = fc.kernel_ms();

  // step 3, sequential by definition: the host replays it over the items of the deficient cameras
  for (size_t t = 0; t < T; ++t) {
    counts[0] += (!point_estimated || point_estimated[t]) && nv[t] >= 1;
    counts[2] += selected_out[t] == 1;
  }
  counts[1] = h_cnt[TS_CELLS];
  const auto t0 = std::chrono::steady_clock::now();
  std::sort(items.begin(), items.end());
  ts_top_up(items.data(), n_list, p.K, selected_out, &counts[3], &counts[4]);
  counts[5] = counts[2] + counts[4];
  if (top_up_out) { top_up_out[0] = (double)n_list; top_up_out[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  if (n_views_out) std::memcpy(n_views_out, nv.data(), T * sizeof(int32_t));
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  return GSFM_OK;
}

}  // namespace
#endif
