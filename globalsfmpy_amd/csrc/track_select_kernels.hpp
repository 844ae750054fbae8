// Device kernels of gsfm_tracks_select_good (include/gsfm_tracks.h; host side: track_select.hpp): Theia's SelectGoodTracksForBundleAdjustment
// under the definition of that header, as data-parallel steps over the estimated tracks and over the n_obs observation places.  An ITEM is an
// observation of an estimated track in an estimated camera; item_track[o] is its track, GSFM_TS_NONE for every other observation place.
//
//   k_track_stats<G>  the lane group, the lane classes and the launch order of k_outlier_tracks<G>, over the estimated tracks: the count n, then
//                     tri_gate<G> alone (no ray store, no angle sweep) for the mean; lane l marks the items it walked in item_track.
//   k_ts_insert       step 2, sweep 1.  The cell table is an open-addressing table of 32-bit slots holding item indices.  A lane claims an
//                     empty slot by CAS; on a taken slot it compares its cell (camera, cx, cy) with the owner's and probes linearly on a
//                     mismatch.  WHICH item owns a cell's slot, and which slot a cell lands in, depend on the race; nothing read afterwards
//                     does: the slot's three minima are taken over ALL items of the cell.  The first is taken here: atomicMin of min(n, L).
//   k_ts_mean         sweep 2: the items whose truncated length is the cell's lower the cell's canonical mean bits (64-bit atomicMin).
//   k_ts_track        sweep 3: the items that match both lower the cell's track index.
//   k_ts_mark         the winners: selected[track] = 1, a plain store of the same value from every writer.
//   k_ts_count        per camera est (items) and opt (items of selected tracks), integer atomics.
//   k_ts_deficient    the items of the cameras with K > 0, opt < K and opt < est, as (camera, track, place) triples behind an atomic cursor:
//                     the list's order is free, the host sorts it before the replay of step 3.
// A kernel boundary separates the sweeps: each reads minima the one before has finished.  Every kernel is a grid-stride loop, every probe loop
// is bounded by the table's size, no work-group waits for another.
#pragma once
#include "triangulate_kernels.hpp"

namespace gsfm {

#define GSFM_TS_NONE 0xffffffffu
#define GSFM_TS_NAN_BITS 0x7ff8000000000000ull

enum TsCounter { TS_ERR = 0, TS_CELLS, TS_LIST, TS_N_COUNTERS = 4 };

struct TsArgs {
  uint32_t n_obs;
  const uint32_t* obs_cam;
  const double2* obs_xy;
  const unsigned long long* track_ptr;
  uint32_t* item_track;          // [n_obs]
  const int32_t* n_views;        // [n_tracks], of k_track_stats
  const double* mean_sq_err;
  double inv_cell;               // 1.0 / S
  uint32_t long_len;             // L
  uint32_t mask;                 // capacity - 1
  uint32_t* table;               // [capacity] owner item, GSFM_TS_NONE = empty
  uint32_t* slot_of;             // [n_obs]
  uint32_t* cell_len;            // [capacity] the three minima of a cell, at its slot
  unsigned long long* cell_mean;
  uint32_t* cell_track;
  uint8_t* selected;             // [n_tracks]
  uint32_t* cam_est;             // [n_cams]
  uint32_t* cam_opt;
  uint32_t min_per_view;         // K
  uint32_t* list;                // [3 x n_obs]
  uint32_t* counters;
};

template <int G>
__global__ void __launch_bounds__(G == 64 ? 64 : GSFM_TRI_BLOCK) k_track_stats(TriArgs a, const double* __restrict__ points, uint32_t* __restrict__ item_track) {
  const int group = threadIdx.x / G, l = threadIdx.x % G, lane_in_wave = threadIdx.x & 63;
  constexpr int GROUPS = (G == 64 ? 64 : GSFM_TRI_BLOCK) / G;
  TriTrack tk;   // tri_track<G> without a ray store: a dead group (the last block's spare slots) runs along on an empty track
  const uint64_t slot = (uint64_t)blockIdx.x * GROUPS + group;
  tk.live = slot < a.n_slots;
  tk.t = tk.live ? a.order[slot] : 0;
  tk.ob = tk.live ? a.track_ptr[tk.t] : 0;
  tk.len = (uint32_t)((tk.live ? a.track_ptr[tk.t + 1] : 0) - tk.ob);
  tk.rx = tk.ry = tk.rz = nullptr;
  double X[3] = {0.0, 0.0, 0.0};
  if (tk.live) { X[0] = points[3 * tk.t]; X[1] = points[3 * tk.t + 1]; X[2] = points[3 * tk.t + 2]; }
  int mine = 0;
  for (uint32_t k = l; k < tk.len; k += G) {
    const bool item = a.cams[(uint64_t)GSFM_TRI_CAM_DOUBLES * a.obs_cam[tk.ob + k] + 15] != 0.0;
    item_track[tk.ob + k] = item ? (uint32_t)tk.t : GSFM_TS_NONE;
    mine += item ? 1 : 0;
  }
  const int n = tri_group_allsum_int<G>(mine);
  double mean;
  (void)tri_gate<G>(a, tk, l, lane_in_wave, X, n, mean);
  if (tk.live && l == 0) { a.n_views[tk.t] = n; a.mean_sq_err[tk.t] = mean; }
}

__device__ __forceinline__ uint32_t ts_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the host has refused every coordinate whose product is not inside the int32 range
__device__ __forceinline__ int32_t ts_cell(double x, double inv) { return (int32_t)(x * inv); }
__device__ __forceinline__ uint32_t ts_hash(uint32_t cam, int32_t cx, int32_t cy) {
  unsigned long long h = ((unsigned long long)(uint32_t)cx << 32 | (uint32_t)cy) * 0x9e3779b97f4a7c15ull;
  h ^= h >> 29;
  h += cam;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  h *= 0x94d049bb133111ebull;
  h ^= h >> 31;
  return (uint32_t)h;
}
__device__ __forceinline__ uint32_t ts_trunc_len(const TsArgs& a, uint32_t t) { const uint32_t n = (uint32_t)a.n_views[t]; return n < a.long_len ? n : a.long_len; }
__device__ __forceinline__ unsigned long long ts_mean_bits(const TsArgs& a, uint32_t t) {
  const double m = a.mean_sq_err[t];
  return m != m ? GSFM_TS_NAN_BITS : (unsigned long long)__double_as_longlong(m);
}

__global__ void __launch_bounds__(256) k_ts_insert(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t == GSFM_TS_NONE) continue;
    const uint32_t cam = a.obs_cam[o];
    const double2 p = a.obs_xy[o];
    const int32_t cx = ts_cell(p.x, a.inv_cell), cy = ts_cell(p.y, a.inv_cell);
    uint32_t slot = ts_hash(cam, cx, cy) & a.mask, found = GSFM_TS_NONE;
    for (uint32_t probe = 0; probe <= a.mask; ++probe, slot = (slot + 1) & a.mask) {
      uint32_t owner = ts_ld(a.table + slot);
      if (owner == GSFM_TS_NONE) {
        owner = atomicCAS(a.table + slot, GSFM_TS_NONE, o);
        if (owner == GSFM_TS_NONE) { atomicAdd(a.counters + TS_CELLS, 1u); found = slot; break; }
      }
      if (owner >= a.n_obs) break;   // (never: a slot holds an item index or GSFM_TS_NONE)
      const double2 q = a.obs_xy[owner];
      if (a.obs_cam[owner] == cam && ts_cell(q.x, a.inv_cell) == cx && ts_cell(q.y, a.inv_cell) == cy) { found = slot; break; }
    }
    if (found == GSFM_TS_NONE) { a.counters[TS_ERR] = 1u; found = 0; }   // (a table with fewer slots than items: the host refuses that capacity)
    else atomicMin(a.cell_len + found, ts_trunc_len(a, t));
    a.slot_of[o] = found;
  }
}

__global__ void __launch_bounds__(256) k_ts_mean(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t == GSFM_TS_NONE) continue;
    const uint32_t slot = a.slot_of[o];
    if (ts_trunc_len(a, t) == a.cell_len[slot]) atomicMin(a.cell_mean + slot, ts_mean_bits(a, t));
  }
}

__global__ void __launch_bounds__(256) k_ts_track(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t == GSFM_TS_NONE) continue;
    const uint32_t slot = a.slot_of[o];
    if (ts_trunc_len(a, t) == a.cell_len[slot] && ts_mean_bits(a, t) == a.cell_mean[slot]) atomicMin(a.cell_track + slot, t);
  }
}

__global__ void __launch_bounds__(256) k_ts_mark(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t != GSFM_TS_NONE && a.cell_track[a.slot_of[o]] == t) a.selected[t] = 1;
  }
}

__global__ void __launch_bounds__(256) k_ts_count(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t == GSFM_TS_NONE) continue;
    const uint32_t cam = a.obs_cam[o];
    atomicAdd(a.cam_est + cam, 1u);
    if (a.selected[t]) atomicAdd(a.cam_opt + cam, 1u);
  }
}

__global__ void __launch_bounds__(256) k_ts_deficient(TsArgs a) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_obs; o += stride) {
    const uint32_t t = a.item_track[o];
    if (t == GSFM_TS_NONE) continue;
    const uint32_t cam = a.obs_cam[o], opt = a.cam_opt[cam];
    if (a.min_per_view == 0 || opt >= a.min_per_view || opt >= a.cam_est[cam]) continue;
    const uint32_t at = atomicAdd(a.counters + TS_LIST, 1u);   // at most one entry per observation place: at < n_obs
    a.list[3 * (uint64_t)at] = cam; a.list[3 * (uint64_t)at + 1] = t; a.list[3 * (uint64_t)at + 2] = (uint32_t)(o - a.track_ptr[t]);
  }
}

}  // namespace gsfm
