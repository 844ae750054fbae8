// Device kernels of gsfm_tracks_build (include/gsfm_tracks.h; host side: track_build.hpp): Theia's TrackBuilder as data-parallel steps over
// the n = 2 n_matches endpoints, the F features and the candidate tracks.  No library sort or hash; integer atomics only.
//
//   k_tb_views       endpoint -> view: a binary search of the match in match_ptr, once
//   k_tb_insert      feature identification: an open-addressing table of 32-bit slots holding endpoint indices.  A lane claims an empty slot
//                    by CAS; on a taken slot it compares its full key (view, both doubles) with the owner's and probes linearly on a
//                    mismatch; on a match it lowers the slot to its own index by atomicMin -- every value a slot ever holds has the slot's
//                    key, so the comparison stays valid, and in the end the slot holds the smallest endpoint with that key whichever lane
//                    won it.  WHICH slot a key lands in depends on the race, nothing read afterwards does.
//   k_tb_rep         representative per endpoint and the flag "is its own representative"
//   k_tb_features    feature id = exclusive prefix sum of that flag (k_scan_*), per endpoint and per feature its representative; label = id
//   k_tb_hook        components: a match whose features' labels differ lowers the larger label's label to the smaller (atomicMin) and raises
//                    the round's "changed" word;  k_tb_jump: every feature follows the labels to a root.  A label only ever decreases and
//                    always names a feature of the same component, so stale reads are harmless (tree_kernels.hpp's argument).  A round
//                    whose hook changes nothing leaves every feature with its component's smallest id.  k_tb_post hands the changed words
//                    to the host through mapped memory and clears them.
//   k_tb_sizes       component sizes by integer atomics;  k_tb_classify: components counted, those larger than max_track_length flagged
//                    for the replay, the min-length filter
//   k_tb_tracks      per candidate track (rank of its label among the kept labels, by scan) its slice of the candidate array (offsets by
//                    scan) and its entry in the list of its lane class;  k_tb_place: features into their track's slice, in any order
//   k_tb_order<G>    one group of G = 4 / 16 / 64 lanes per track (the classes of track_scene.hpp by track length; lengths above 64 loop):
//                    an item's place is the number of items of the track with a smaller feature id -- stable by construction -- and it is a
//                    duplicate when a smaller feature id of the track has its view
//   k_tb_emit_*      compaction to the final CSR by scans over "observation kept" and "track kept"
// Every kernel is a grid-stride loop over a count it reads from device memory where the host does not know it yet.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsfm {

#define GSFM_TB_EMPTY 0xffffffffu
#define GSFM_TB_SCAN_ITEMS 8
#define GSFM_TB_SCAN_TILE (256 * GSFM_TB_SCAN_ITEMS)

// the call's device counters
enum TbCounter { TB_ERR = 0, TB_FEATURES, TB_COMPONENTS, TB_SMALL, TB_BIG, TB_INCONSISTENT, TB_DEGENERATE, TB_CLASS0, TB_CLASS1, TB_CLASS2, TB_CAND_TRACKS,
                 TB_CAND_OBS, TB_TRACKS, TB_OBS, TB_N_COUNTERS = 16 };

__device__ __forceinline__ uint32_t tb_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// -0.0 and 0.0 are one key: x + 0.0 is +0.0 for both
__device__ __forceinline__ uint32_t tb_hash(uint32_t view, double x, double y) {
  unsigned long long h = (unsigned long long)__double_as_longlong(x + 0.0) * 0x9e3779b97f4a7c15ull;
  h ^= h >> 29;
  h += (unsigned long long)__double_as_longlong(y + 0.0);
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  h += view;
  h *= 0x94d049bb133111ebull;
  h ^= h >> 31;
  return (uint32_t)h;
}

__global__ void __launch_bounds__(256) k_tb_views(uint64_t n_edges, const uint64_t* __restrict__ match_ptr, const uint32_t* __restrict__ edge_i,
                                                  const uint32_t* __restrict__ edge_j, uint32_t n_matches, uint32_t* __restrict__ eview) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < n_matches; m += stride) {
    uint64_t lo = 0, hi = n_edges;   // the last edge with match_ptr[e] <= m (empty edges share an offset: the last of them holds the match)
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) / 2; if (match_ptr[mid] <= m) lo = mid; else hi = mid; }
    eview[2 * m] = edge_i[lo]; eview[2 * m + 1] = edge_j[lo];
  }
}

__global__ void __launch_bounds__(256) k_tb_insert(uint32_t n, const uint32_t* __restrict__ eview, const double2* __restrict__ xy, uint32_t* table,
                                                   uint32_t mask, uint32_t* __restrict__ slot_of, uint32_t* counters) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t v = eview[e];
    const double2 p = xy[e];
    uint32_t slot = tb_hash(v, p.x, p.y) & mask, found = GSFM_TB_EMPTY;
    for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
      uint32_t owner = tb_ld(table + slot);
      if (owner == GSFM_TB_EMPTY) {
        owner = atomicCAS(table + slot, GSFM_TB_EMPTY, e);
        if (owner == GSFM_TB_EMPTY) { found = slot; break; }
      }
      const double2 q = xy[owner];
      if (eview[owner] == v && q.x == p.x && q.y == p.y) { atomicMin(table + slot, e); found = slot; break; }
    }
    if (found == GSFM_TB_EMPTY) { counters[TB_ERR] = 1; found = 0; }   // (a table with fewer slots than keys: the host refuses that capacity)
    slot_of[e] = found;
  }
}

// slot_of becomes the representative, in place
__global__ void __launch_bounds__(256) k_tb_rep(uint32_t n, const uint32_t* __restrict__ table, uint32_t* __restrict__ rep, uint32_t* __restrict__ is_rep) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    uint32_t r = table[rep[e]];
    if (r >= n) r = e;   // (only after an overflow, which the host reports: keep every index in range)
    rep[e] = r; is_rep[e] = r == e ? 1u : 0u;
  }
}

// ---- exclusive prefix sum of n 32-bit counts (n from the host, or *n_dev when n_dev is given): tile sums, their scan by one block, the tiles ----
__device__ __forceinline__ uint32_t tb_block_exclusive(uint32_t v, uint32_t* lds, uint32_t* total) {   // 256 lanes; lds: 256 words
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const uint32_t add = t >= off ? lds[t - off] : 0u;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const uint32_t incl = lds[t];
  *total = lds[255];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(256) k_scan_tiles(const uint32_t* __restrict__ in, uint32_t n_host, const uint32_t* n_dev, uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t lds[256];
  const uint32_t n = n_dev ? *n_dev : n_host, n_tiles = (n + GSFM_TB_SCAN_TILE - 1) / GSFM_TB_SCAN_TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t base = tile * GSFM_TB_SCAN_TILE + threadIdx.x * GSFM_TB_SCAN_ITEMS;
    uint32_t s = 0;
    for (int k = 0; k < GSFM_TB_SCAN_ITEMS; ++k) if (base + k < n) s += in[base + k];
    uint32_t total;
    (void)tb_block_exclusive(s, lds, &total);
    if (threadIdx.x == 0) tile_sum[tile] = total;
  }
}
// one block: tile_sum becomes its exclusive scan; the grand total goes to *total_out
__global__ void __launch_bounds__(256) k_scan_sums(uint32_t* tile_sum, uint32_t n_host, const uint32_t* n_dev, uint32_t* total_out) {
  __shared__ uint32_t lds[256];
  const uint32_t n = n_dev ? *n_dev : n_host, n_tiles = (n + GSFM_TB_SCAN_TILE - 1) / GSFM_TB_SCAN_TILE;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_tiles; base += 256) {   // block-uniform trip count
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_tiles ? tile_sum[i] : 0u;
    uint32_t total;
    const uint32_t ex = tb_block_exclusive(v, lds, &total);
    if (i < n_tiles) tile_sum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}
__global__ void __launch_bounds__(256) k_scan_apply(const uint32_t* __restrict__ in, uint32_t n_host, const uint32_t* n_dev, const uint32_t* __restrict__ tile_sum,
                                                    uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[256];
  const uint32_t n = n_dev ? *n_dev : n_host, n_tiles = (n + GSFM_TB_SCAN_TILE - 1) / GSFM_TB_SCAN_TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t base = tile * GSFM_TB_SCAN_TILE + threadIdx.x * GSFM_TB_SCAN_ITEMS;
    uint32_t v[GSFM_TB_SCAN_ITEMS], s = 0;
    for (int k = 0; k < GSFM_TB_SCAN_ITEMS; ++k) { v[k] = base + k < n ? in[base + k] : 0u; s += v[k]; }
    uint32_t total;
    uint32_t run = tile_sum[tile] + tb_block_exclusive(s, lds, &total);
    for (int k = 0; k < GSFM_TB_SCAN_ITEMS; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
  }
}

// fscan: the exclusive scan of is_rep.  efeat: feature id per endpoint; feat_ep: representative per feature; label starts as the id.
__global__ void __launch_bounds__(256) k_tb_features(uint32_t n, const uint32_t* __restrict__ rep, const uint32_t* __restrict__ fscan, uint32_t* __restrict__ efeat,
                                                     uint32_t* __restrict__ feat_ep, uint32_t* __restrict__ label) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t r = rep[e], f = fscan[r];
    efeat[e] = f;
    if (r == e) { feat_ep[f] = e; label[f] = f; }
  }
}

__global__ void __launch_bounds__(256) k_tb_hook(uint32_t n_matches, const uint32_t* __restrict__ efeat, uint32_t* label, uint32_t* changed) {
  const uint32_t stride = gridDim.x * blockDim.x;
  bool any = false;
  for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < n_matches; m += stride) {
    const uint32_t a = tb_ld(label + efeat[2 * m]), b = tb_ld(label + efeat[2 * m + 1]);
    if (a != b) { any = true; atomicMin(label + (a > b ? a : b), a > b ? b : a); }
  }
  if (any) *changed = 1u;
}
__global__ void __launch_bounds__(256) k_tb_jump(const uint32_t* n_features, uint32_t* label) {
  const uint32_t n = *n_features, stride = gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
    uint32_t p = tb_ld(label + f), q = tb_ld(label + p);
    if (p == q) continue;
    while (p != q) { p = q; q = tb_ld(label + p); }   // labels decrease along the way: the walk ends at a root
    __hip_atomic_store(label + f, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// the host's look: n words to mapped host memory, the stamp after them, the device words cleared for the next rounds
__global__ void k_tb_post(uint32_t* words, int n, uint32_t* mail, uint32_t stamp) {
  for (int k = 0; k < n; ++k) { mail[k] = words[k]; words[k] = 0u; }
  __hip_atomic_store(mail + n, stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(256) k_tb_sizes(const uint32_t* n_features, const uint32_t* __restrict__ label, uint32_t* size) {
  const uint32_t n = *n_features, stride = gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) atomicAdd(size + label[f], 1u);
}
// per feature: keep = 1 for the label of a candidate track, keep_size = its size there (0 elsewhere); is_big = 1 for a label that goes to the replay
__global__ void __launch_bounds__(256) k_tb_classify(const uint32_t* n_features, const uint32_t* __restrict__ label, const uint32_t* __restrict__ size, uint32_t min_len,
                                                     uint32_t max_len, uint32_t* __restrict__ keep, uint32_t* __restrict__ keep_size, uint32_t* __restrict__ is_big,
                                                     uint32_t* counters) {
  const uint32_t n = *n_features, stride = gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
    const bool root = label[f] == f;
    const uint32_t s = root ? size[f] : 0u;
    const bool big = root && s > max_len, small = root && s < min_len;
    keep[f] = root && !small ? 1u : 0u;
    keep_size[f] = root && !small ? s : 0u;
    if (is_big) is_big[f] = big ? 1u : 0u;
    if (root) atomicAdd(counters + TB_COMPONENTS, 1u);
    if (small) atomicAdd(counters + TB_SMALL, 1u);
    if (big) atomicAdd(counters + TB_BIG, 1u);
  }
}

// trank / toff: the exclusive scans of keep / keep_size.  Lane classes by track length as in track_scene.hpp: <= 8, <= 64, longer.
__global__ void __launch_bounds__(256) k_tb_tracks(const uint32_t* n_features, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ keep_size,
                                                   const uint32_t* __restrict__ trank, const uint32_t* __restrict__ toff, uint32_t* __restrict__ cbase,
                                                   uint32_t* __restrict__ clen, uint32_t* __restrict__ cursor, uint32_t* __restrict__ list0, uint32_t* __restrict__ list1,
                                                   uint32_t* __restrict__ list2, uint32_t* counters) {
  const uint32_t n = *n_features, stride = gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
    if (!keep[f]) continue;
    const uint32_t t = trank[f], len = keep_size[f];
    cbase[t] = toff[f]; clen[t] = len; cursor[t] = 0u;
    if (len <= 8) list0[atomicAdd(counters + TB_CLASS0, 1u)] = t;
    else if (len <= 64) list1[atomicAdd(counters + TB_CLASS1, 1u)] = t;
    else list2[atomicAdd(counters + TB_CLASS2, 1u)] = t;
  }
}
__global__ void __launch_bounds__(256) k_tb_place(const uint32_t* n_features, const uint32_t* __restrict__ label, const uint32_t* __restrict__ keep,
                                                  const uint32_t* __restrict__ trank, const uint32_t* __restrict__ cbase, uint32_t* cursor, uint32_t* __restrict__ cand) {
  const uint32_t n = *n_features, stride = gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
    const uint32_t r = label[f];
    if (!keep[r]) continue;
    const uint32_t t = trank[r];
    cand[cbase[t] + atomicAdd(cursor + t, 1u)] = f;
  }
}

// One group of G lanes per track of the class's list.  Two walks over the track's items, lane l taking the items l, l + G, ...: the first counts
// the duplicates (so that the track's fate is known before anything is written), the second writes each item to its place.
template <int G>
__global__ void __launch_bounds__(G == 64 ? 64 : 256) k_tb_order(const uint32_t* __restrict__ list, const uint32_t* n_list, const uint32_t* __restrict__ cbase,
                                                                 const uint32_t* __restrict__ clen, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ feat_ep,
                                                                 const uint32_t* __restrict__ eview, uint32_t* __restrict__ sorted, uint32_t* __restrict__ ok,
                                                                 uint32_t* __restrict__ valid, uint32_t* counters) {
  const uint32_t groups_per_block = blockDim.x / G, lane = threadIdx.x % G, n = *n_list;
  const uint32_t first = blockIdx.x * groups_per_block + threadIdx.x / G, stride = gridDim.x * groups_per_block;
  const uint32_t rounds = (n + stride - 1) / stride;   // every lane runs the same number of rounds: the shuffles below stay wave-uniform
  for (uint32_t round = 0; round < rounds; ++round) {
    const uint32_t slot = first + round * stride;
    const bool live = slot < n;
    const uint32_t t = live ? list[slot] : 0u, base = live ? cbase[t] : 0u, len = live ? clen[t] : 0u;
    uint32_t n_dup = 0;   // (a dead group has len = 0 and walks nothing; the lanes meet again at the shuffles)
    for (uint32_t i = lane; i < len; i += G) {
      const uint32_t f = cand[base + i], v = eview[feat_ep[f]];
      bool dup = false;
      for (uint32_t j = 0; j < len; ++j) { const uint32_t g = cand[base + j]; dup |= g < f && eview[feat_ep[g]] == v; }
      n_dup += dup ? 1u : 0u;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) n_dup += __shfl_xor(n_dup, off, 64);
    const bool good = len - n_dup >= 2;
    for (uint32_t i = lane; i < len; i += G) {
      const uint32_t f = cand[base + i], v = eview[feat_ep[f]];
      uint32_t place = 0;
      bool dup = false;
      for (uint32_t j = 0; j < len; ++j) { const uint32_t g = cand[base + j]; place += g < f ? 1u : 0u; dup |= g < f && eview[feat_ep[g]] == v; }
      sorted[base + place] = f;
      ok[base + place] = good && !dup ? 1u : 0u;
    }
    if (live && lane == 0) {
      valid[t] = good ? 1u : 0u;
      if (n_dup) atomicAdd(counters + TB_INCONSISTENT, n_dup);
      if (!good) atomicAdd(counters + TB_DEGENERATE, 1u);
    }
  }
}

// dest: the exclusive scan of ok over the candidate observations
__global__ void __launch_bounds__(256) k_tb_emit_obs(const uint32_t* n_cand_obs, const uint32_t* __restrict__ ok, const uint32_t* __restrict__ dest,
                                                     const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ feat_ep, const uint32_t* __restrict__ eview,
                                                     const double2* __restrict__ xy, uint32_t* __restrict__ obs_view, double2* __restrict__ obs_xy) {
  const uint32_t n = *n_cand_obs, stride = gridDim.x * blockDim.x;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += stride) {
    if (!ok[s]) continue;
    const uint32_t e = feat_ep[sorted[s]], d = dest[s];
    obs_view[d] = eview[e]; obs_xy[d] = xy[e];
  }
}
// frank: the exclusive scan of valid over the candidate tracks
__global__ void __launch_bounds__(256) k_tb_emit_ptr(const uint32_t* n_cand_tracks, const uint32_t* __restrict__ valid, const uint32_t* __restrict__ frank,
                                                     const uint32_t* __restrict__ cbase, const uint32_t* __restrict__ dest, const uint32_t* counters,
                                                     unsigned long long* __restrict__ track_ptr) {
  const uint32_t n = *n_cand_tracks, stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride)
    if (valid[t]) track_ptr[frank[t]] = dest[cbase[t]];
  if (blockIdx.x == 0 && threadIdx.x == 0) track_ptr[counters[TB_TRACKS]] = counters[TB_OBS];
}

}  // namespace gsfm
