// gsfm_tracks_build and gsfm_tracks_build_sequential (include/gsfm_tracks.h): tracks from two-view matches, Theia's TrackBuilder.
// Plain C++ first (no HIP: a host compiler alone builds it, as it builds lm_loop.hpp and the first half of track_scene.hpp): the argument checks,
// Theia's union rule, the sequential restatement over all matches and the replay of the components larger than max_track_length.  Under hipcc: the
// host side of the device call on the scratch owner of flat_call.hpp, launching track_build_kernels.hpp.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "track_scene.hpp"
#include "../../include/gsfm_tracks.h"

namespace {

struct TbOptions { uint32_t min_len = 2, max_len = 1000; int capacity_log2 = 0; };
constexpr uint64_t TB_MAX_MATCHES = 1ull << 29;
constexpr uint32_t TB_NONE = 0xffffffffu;

// the smallest capacity the table may have, and the one it gets by default (log2)
inline int tb_min_capacity_log2(uint64_t n_matches) { int k = 0; while ((1ull << k) < 2 * n_matches) ++k; return k; }
inline int tb_auto_capacity_log2(uint64_t n_matches) { return std::max(10, tb_min_capacity_log2(n_matches) + 1); }

// Every check of the entry, in the order it reports them; fills *o.  false: *why
inline bool tb_args_ok(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr, const double* matches,
                       const gsfm_tracks_build_options* options, const uint64_t* track_ptr_out, const uint32_t* obs_view_out, const double* obs_xy_out,
                       const uint64_t* n_tracks, const uint64_t* n_obs, TbOptions* o, std::string* why) {
  auto refuse = [why](const std::string& message) { *why = message; return false; };
  if (!track_ptr_out || !n_tracks || !n_obs) return refuse("NULL argument");
  if (options) {
    if (options->min_track_length < 1 || options->max_track_length < 1) return refuse("min_track_length and max_track_length must be at least 1");
    if (options->hash_capacity_log2 < 0 || options->hash_capacity_log2 > 31) return refuse("hash_capacity_log2 must be 0 (automatic) or at most 31");
    o->min_len = (uint32_t)options->min_track_length; o->max_len = (uint32_t)options->max_track_length; o->capacity_log2 = options->hash_capacity_log2;
  }
  if (n_edges == 0) return true;
  if (!edge_i || !edge_j) return refuse("NULL argument");
  if (!track_ptr_ok(n_edges, match_ptr, TrackLimit::tracks, 0, true, "NULL argument", why)) { *why = "match_ptr (as a track_ptr over the edges): " + *why; return false; }
  const uint64_t M = match_ptr[n_edges];
  if (M > TB_MAX_MATCHES) return refuse("problem too large (more than 2^29 matches)");
  for (uint64_t e = 0; e < n_edges; ++e)
    if (edge_i[e] >= n_views || edge_j[e] >= n_views || edge_i[e] == edge_j[e])
      return refuse("edge " + std::to_string(e) + " has an out-of-range view index or joins a view to itself");
  if (M == 0) return true;
  if (!matches || !obs_view_out || !obs_xy_out) return refuse("NULL argument");
  for (uint64_t k = 0; k < 4 * M; ++k) if (!std::isfinite(matches[k])) return refuse("match " + std::to_string(k / 4) + " has a coordinate that is not finite");
  if (o->capacity_log2 != 0 && o->capacity_log2 < tb_min_capacity_log2(M))
    return refuse("hash_capacity_log2 = " + std::to_string(o->capacity_log2) + " gives fewer slots than the " + std::to_string(2 * M) + " endpoints");
  return true;
}

// Theia's ConnectedComponents::AddEdge (math/graph/connected_components.h:87-108) over dense ids: nothing happens when both nodes share a root or when
// the two sizes add up to more than the maximum; else the smaller tree goes under the larger, the first node's under the second's only when it is smaller
struct TheiaComponents {
  std::vector<uint32_t> parent, size;
  uint64_t max_size;
  bool refused = false;
  TheiaComponents(size_t n, uint64_t max_size_) : parent(n), size(n, 1), max_size(max_size_) { for (size_t k = 0; k < n; ++k) parent[k] = (uint32_t)k; }
  uint32_t find(uint32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  }
  void add_edge(uint32_t a, uint32_t b) {
    const uint32_t ra = find(a), rb = find(b);
    if (ra == rb) return;
    if ((uint64_t)size[ra] + size[rb] > max_size) { refused = true; return; }
    if (size[ra] < size[rb]) { parent[ra] = rb; size[rb] += size[ra]; }
    else { parent[rb] = ra; size[ra] += size[rb]; }
  }
  // label[f] = the smallest id of f's component, for the ids `in` selects
  template <typename In> void labels(In in, uint32_t* label) {
    std::vector<uint32_t> smallest(parent.size(), TB_NONE);
    for (size_t f = 0; f < parent.size(); ++f) {
      if (!in(f)) continue;
      const uint32_t r = find((uint32_t)f);
      if (smallest[r] == TB_NONE) smallest[r] = (uint32_t)f;
      label[f] = smallest[r];
    }
  }
};

// The replay: the matches whose component is flagged (is_big, by plain label) run through Theia's rule in the caller's order; their features are relabelled
inline void tb_replay(uint64_t n_matches, const uint32_t* efeat, size_t n_features, uint32_t* label, const uint32_t* is_big, uint32_t max_len) {
  TheiaComponents cc(n_features, max_len);
  for (uint64_t m = 0; m < n_matches; ++m)
    if (is_big[label[efeat[2 * m]]]) cc.add_edge(efeat[2 * m], efeat[2 * m + 1]);
  std::vector<uint8_t> in(n_features);
  for (size_t f = 0; f < n_features; ++f) in[f] = is_big[label[f]] != 0;
  cc.labels([&in](size_t f) { return in[f] != 0; }, label);
}

struct TbKey {
  uint32_t view; uint64_t x, y;
  bool operator==(const TbKey& k) const { return view == k.view && x == k.x && y == k.y; }
};
struct TbKeyHash {
  size_t operator()(const TbKey& k) const {
    uint64_t h = k.x * 0x9e3779b97f4a7c15ull; h ^= h >> 29; h += k.y; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32; h += k.view; h *= 0x94d049bb133111ebull;
    return (size_t)(h ^ (h >> 31));
  }
};
inline uint64_t tb_bits(double v) { v += 0.0; uint64_t b; std::memcpy(&b, &v, 8); return b; }   // -0.0 + 0.0 = +0.0: one key for both zeros

// The definition, sequentially (arguments checked by the caller; n_matches > 0)
inline void tb_sequential(uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr, const double* matches, const TbOptions& o,
                          uint64_t* track_ptr_out, uint32_t* obs_view_out, double* obs_xy_out, uint64_t* n_tracks, uint64_t* n_obs, uint64_t counts[7]) {
  const uint64_t M = match_ptr[n_edges];
  std::unordered_map<TbKey, uint32_t, TbKeyHash> ids;
  ids.reserve((size_t)(2 * M));
  std::vector<uint32_t> efeat((size_t)(2 * M)), feat_ep, feat_view;
  for (uint64_t e = 0; e < n_edges; ++e)
    for (uint64_t m = match_ptr[e]; m < match_ptr[e + 1]; ++m)
      for (int side = 0; side < 2; ++side) {
        const uint32_t view = side ? edge_j[e] : edge_i[e];
        const TbKey key{view, tb_bits(matches[4 * m + 2 * side]), tb_bits(matches[4 * m + 2 * side + 1])};
        const auto it = ids.emplace(key, (uint32_t)feat_ep.size());
        if (it.second) { feat_ep.push_back((uint32_t)(2 * m + side)); feat_view.push_back(view); }
        efeat[2 * m + side] = it.first->second;
      }
  const size_t F = feat_ep.size();
  TheiaComponents cc(F, o.max_len);
  for (uint64_t m = 0; m < M; ++m) cc.add_edge(efeat[2 * m], efeat[2 * m + 1]);
  uint64_t replayed = 0;
  if (cc.refused) {   // the plain components larger than the maximum, for the count alone
    TheiaComponents plain(F, ~0ull);
    for (uint64_t m = 0; m < M; ++m) plain.add_edge(efeat[2 * m], efeat[2 * m + 1]);
    for (size_t f = 0; f < F; ++f) replayed += plain.parent[f] == f && plain.size[f] > o.max_len;
  }
  std::vector<uint32_t> label(F);
  cc.labels([](size_t) { return true; }, label.data());
  // members by label in ascending feature id: a counting sort by label
  std::vector<uint32_t> start(F + 1, 0), member(F);
  for (size_t f = 0; f < F; ++f) ++start[label[f] + 1];
  for (size_t f = 0; f < F; ++f) start[f + 1] += start[f];
  { std::vector<uint32_t> fill(start.begin(), start.end() - 1); for (size_t f = 0; f < F; ++f) member[fill[label[f]]++] = (uint32_t)f; }
  uint64_t T = 0, O = 0, components = 0, small = 0, inconsistent = 0, degenerate = 0;
  track_ptr_out[0] = 0;
  std::vector<uint32_t> seen_in(*std::max_element(feat_view.begin(), feat_view.end()) + (size_t)1, TB_NONE);   // view -> the last label it was seen in
  for (size_t l = 0; l < F; ++l) {
    const uint32_t len = start[l + 1] - start[l];
    if (len == 0) continue;
    ++components;
    if (len < o.min_len) { ++small; continue; }
    uint64_t kept = 0;
    for (uint32_t k = start[l]; k < start[l + 1]; ++k) {
      const uint32_t f = member[k], v = feat_view[f];
      if (seen_in[v] == (uint32_t)l) { ++inconsistent; continue; }
      seen_in[v] = (uint32_t)l;
      obs_view_out[O + kept] = v;
      obs_xy_out[2 * (O + kept)] = matches[2 * (uint64_t)feat_ep[f]]; obs_xy_out[2 * (O + kept) + 1] = matches[2 * (uint64_t)feat_ep[f] + 1];
      ++kept;
    }
    if (kept < 2) { ++degenerate; continue; }
    O += kept;
    track_ptr_out[++T] = O;
  }
  *n_tracks = T; *n_obs = O;
  const uint64_t c[7] = {F, components, small, inconsistent, degenerate, replayed, T};
  std::memcpy(counts, c, sizeof(c));
}

}  // namespace

#ifdef __HIPCC__
#include "flat_call.hpp"
#include "track_build_kernels.hpp"

namespace {

// The host's look at a few device words without a stream synchronisation: k_tb_post writes them to mapped host memory, an event behind it tells the host
struct TbMail {
  uint32_t* host = nullptr; uint32_t* dev = nullptr;
  hipEvent_t ev = nullptr;
  uint32_t stamp = 0;
  static constexpr int WORDS = 2;
  ~TbMail() { if (ev) (void)hipEventDestroy(ev); if (host) (void)hipHostFree(host); }
  int open() {
    HIPCHK(hipHostMalloc((void**)&host, (WORDS + 1) * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(host, 0, (WORDS + 1) * sizeof(uint32_t));
    HIPCHK(hipHostGetDevicePointer((void**)&dev, host, 0));
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return 0;
  }
  // enqueue the post of `words` and wait for it; out[WORDS]
  int look(hipStream_t s, uint32_t* words, uint32_t* out) {
    hipLaunchKernelGGL(k_tb_post, dim3(1), dim3(1), 0, s, words, (int)WORDS, dev, ++stamp);
    HIPCHK(hipEventRecord(ev, s));
    HIPCHK(hipEventSynchronize(ev));
    if (__atomic_load_n(host + WORDS, __ATOMIC_ACQUIRE) != stamp) return fail(GSFM_ERR_HIP, "the track builder's component rounds never reported");
    for (int k = 0; k < WORDS; ++k) out[k] = host[k];
    return 0;
  }
};

gsfm_status tracks_build_sequential_impl(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr, const double* matches,
                                         const gsfm_tracks_build_options* options, uint64_t* track_ptr_out, uint32_t* obs_view_out, double* obs_xy_out, uint64_t* n_tracks,
                                         uint64_t* n_obs, uint64_t* counts_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  TbOptions o;
  std::string why;
  if (!tb_args_ok(n_views, n_edges, edge_i, edge_j, match_ptr, matches, options, track_ptr_out, obs_view_out, obs_xy_out, n_tracks, n_obs, &o, &why))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
  *n_tracks = 0; *n_obs = 0; track_ptr_out[0] = 0;
  if (n_edges == 0 || match_ptr[n_edges] == 0) return GSFM_OK;
  tb_sequential(n_edges, edge_i, edge_j, match_ptr, matches, o, track_ptr_out, obs_view_out, obs_xy_out, n_tracks, n_obs, counts);
  if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
  return GSFM_OK;
}

gsfm_status tracks_build_impl(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr, const double* matches,
                              const gsfm_tracks_build_options* options, uint64_t* track_ptr_out, uint32_t* obs_view_out, double* obs_xy_out, uint64_t* n_tracks,
                              uint64_t* n_obs, uint64_t* counts_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (counts_out) for (int k = 0; k < 7; ++k) counts_out[k] = 0;
  TbOptions o;
  std::string why;
  if (!tb_args_ok(n_views, n_edges, edge_i, edge_j, match_ptr, matches, options, track_ptr_out, obs_view_out, obs_xy_out, n_tracks, n_obs, &o, &why))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
  *n_tracks = 0; *n_obs = 0; track_ptr_out[0] = 0;
  if (n_edges == 0 || match_ptr[n_edges] == 0) return GSFM_OK;   // no matches: no track
  if (const char* reason = no_device_reason("the track builder")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, reason);

  const size_t E = n_edges, M = match_ptr[n_edges], n = 2 * M;
  const int cap_log2 = o.capacity_log2 ? o.capacity_log2 : tb_auto_capacity_log2(M);
  const size_t capacity = (size_t)1 << cap_log2, n_tiles = (n + GSFM_TB_SCAN_TILE - 1) / GSFM_TB_SCAN_TILE;
  FlatLayout L;
  const auto s_ei = L.take<uint32_t>(E), s_ej = L.take<uint32_t>(E); const auto s_mp = L.take<uint64_t>(E + 1); const auto s_xy = L.take<double2>(n);
  const auto s_table = L.take<uint32_t>(capacity), s_cnt = L.take<uint32_t>(TB_N_COUNTERS), s_changed = L.take<uint32_t>(TbMail::WORDS), s_tile = L.take<uint32_t>(n_tiles);
  // per endpoint; per feature (F <= n); per candidate track and candidate observation (both <= F)
  const auto s_eview = L.take<uint32_t>(n), s_rep = L.take<uint32_t>(n), s_isrep = L.take<uint32_t>(n), s_fscan = L.take<uint32_t>(n), s_efeat = L.take<uint32_t>(n);
  const auto s_fep = L.take<uint32_t>(n), s_label = L.take<uint32_t>(n), s_size = L.take<uint32_t>(n), s_keep = L.take<uint32_t>(n), s_ksize = L.take<uint32_t>(n),
             s_big = L.take<uint32_t>(n), s_trank = L.take<uint32_t>(n), s_toff = L.take<uint32_t>(n);
  const auto s_cbase = L.take<uint32_t>(n), s_clen = L.take<uint32_t>(n), s_cursor = L.take<uint32_t>(n), s_valid = L.take<uint32_t>(n), s_frank = L.take<uint32_t>(n),
             s_list0 = L.take<uint32_t>(n), s_list1 = L.take<uint32_t>(n), s_list2 = L.take<uint32_t>(n);
  const auto s_cand = L.take<uint32_t>(n), s_sorted = L.take<uint32_t>(n), s_ok = L.take<uint32_t>(n), s_dest = L.take<uint32_t>(n);
  const auto s_oview = L.take<uint32_t>(n); const auto s_oxy = L.take<double2>(n); const auto s_optr = L.take<unsigned long long>(M + 1);
  FlatCall fc;
  if (int st = fc.commit(L, "the track builder", 3)) return (gsfm_status)st;
  TbMail mail;
  if (int st = mail.open()) return (gsfm_status)st;
  const hipStream_t s = fc.s;
  HIPCHK_S(fc.upload(s_ei, edge_i, E)); HIPCHK_S(fc.upload(s_ej, edge_j, E)); HIPCHK_S(fc.upload(s_mp, match_ptr, E + 1)); HIPCHK_S(fc.upload(s_xy, matches, n));
  HIPCHK_S(hipMemsetAsync(fc.ptr(s_table), 0xff, 4 * capacity, s));
  HIPCHK_S(fc.zero(s_cnt, (size_t)TB_N_COUNTERS)); HIPCHK_S(fc.zero(s_changed, (size_t)TbMail::WORDS)); HIPCHK_S(fc.zero(s_size, n));

  uint32_t* cnt = fc.ptr(s_cnt);
  const uint32_t* eview = fc.ptr(s_eview); const uint32_t* fep = fc.ptr(s_fep); const double2* xy = fc.ptr(s_xy);
  uint32_t* label = fc.ptr(s_label); uint32_t* tile = fc.ptr(s_tile);
  const uint32_t* n_feat = cnt + TB_FEATURES;
  const dim3 blk(256);
  auto grid = [](size_t count, size_t per_block = 256) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((count + per_block - 1) / per_block, 16384))); };
  // out = the exclusive prefix sum of `in` over *count_dev entries (at most `bound`; count_dev NULL: exactly bound), the total to *total
  auto scan = [&](const uint32_t* in, size_t bound, const uint32_t* count_dev, uint32_t* out, uint32_t* total) {
    const dim3 g = grid(bound, GSFM_TB_SCAN_TILE);
    hipLaunchKernelGGL(k_scan_tiles, g, blk, 0, s, in, (uint32_t)bound, count_dev, tile);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), blk, 0, s, tile, (uint32_t)bound, count_dev, total);
    hipLaunchKernelGGL(k_scan_apply, g, blk, 0, s, in, (uint32_t)bound, count_dev, (const uint32_t*)tile, out);
  };
  uint32_t h_cnt[TB_N_COUNTERS];
  auto read_counters = [&]() -> int {
    HIPCHK(fc.download(h_cnt, s_cnt, (size_t)TB_N_COUNTERS));
    HIPCHK(fc.sync());
    return 0;
  };
  auto sizes_and_filter = [&](uint32_t max_len, uint32_t* is_big) {
    hipLaunchKernelGGL(k_tb_sizes, grid(n), blk, 0, s, n_feat, (const uint32_t*)label, fc.ptr(s_size));
    hipLaunchKernelGGL(k_tb_classify, grid(n), blk, 0, s, n_feat, (const uint32_t*)label, (const uint32_t*)fc.ptr(s_size), o.min_len, max_len, fc.ptr(s_keep),
                       fc.ptr(s_ksize), is_big, cnt);
  };

  // ---- span 1: features, plain components, sizes -----------------------------------------------------------------------------------
  HIPCHK_S(fc.begin_span());
  hipLaunchKernelGGL(k_tb_views, grid(M), blk, 0, s, (uint64_t)E, (const uint64_t*)fc.ptr(s_mp), (const uint32_t*)fc.ptr(s_ei), (const uint32_t*)fc.ptr(s_ej), (uint32_t)M,
                     fc.ptr(s_eview));
  hipLaunchKernelGGL(k_tb_insert, grid(n), blk, 0, s, (uint32_t)n, eview, xy, fc.ptr(s_table), (uint32_t)(capacity - 1), fc.ptr(s_rep), cnt);
  hipLaunchKernelGGL(k_tb_rep, grid(n), blk, 0, s, (uint32_t)n, (const uint32_t*)fc.ptr(s_table), fc.ptr(s_rep), fc.ptr(s_isrep));
  scan(fc.ptr(s_isrep), n, nullptr, fc.ptr(s_fscan), cnt + TB_FEATURES);
  hipLaunchKernelGGL(k_tb_features, grid(n), blk, 0, s, (uint32_t)n, (const uint32_t*)fc.ptr(s_rep), (const uint32_t*)fc.ptr(s_fscan), fc.ptr(s_efeat), fc.ptr(s_fep), label);
  // rounds in pairs; the host looks at each pair's "changed" words through the mailbox.  A round whose hook changed nothing ends the loop.
  bool converged = false;
  for (int look = 0; look < 1000 && !converged; ++look) {
    for (int r = 0; r < TbMail::WORDS; ++r) {
      hipLaunchKernelGGL(k_tb_hook, grid(M), blk, 0, s, (uint32_t)M, (const uint32_t*)fc.ptr(s_efeat), label, fc.ptr(s_changed) + r);
      hipLaunchKernelGGL(k_tb_jump, grid(n), blk, 0, s, n_feat, label);
    }
    uint32_t changed[TbMail::WORDS];
    if (int st = mail.look(s, fc.ptr(s_changed), changed)) return (gsfm_status)st;
    for (int r = 0; r < TbMail::WORDS; ++r) converged |= changed[r] == 0;
  }
  if (!converged) return (gsfm_status)fail(GSFM_ERR_HIP, "the track builder's components did not settle in 2000 rounds");
  sizes_and_filter(o.max_len, fc.ptr(s_big));
  HIPCHK_S(fc.end_span());
  if (int st = read_counters()) return (gsfm_status)st;
  if (h_cnt[TB_ERR]) return (gsfm_status)fail(GSFM_ERR_HIP, "the track builder's feature table overflowed");
  const size_t F = h_cnt[TB_FEATURES];
  const uint64_t replayed = h_cnt[TB_BIG];

  // ---- the replay of the components larger than max_track_length, on the host (rare); span 2: the final sizes, the filter, ranks and offsets ----
  if (replayed) {
    hvec<uint32_t> efeat(n), lab(F), big(F);
    HIPCHK_S(fc.download(efeat.data(), s_efeat, n)); HIPCHK_S(fc.download(lab.data(), s_label, F)); HIPCHK_S(fc.download(big.data(), s_big, F));
    HIPCHK_S(fc.sync());
    tb_replay(M, efeat.data(), F, lab.data(), big.data(), o.max_len);
    HIPCHK_S(fc.upload(s_label, lab.data(), F));
    HIPCHK_S(fc.zero(s_size, F));
    h_cnt[TB_COMPONENTS] = h_cnt[TB_SMALL] = h_cnt[TB_BIG] = 0;
    HIPCHK_S(fc.upload(s_cnt, h_cnt, (size_t)TB_N_COUNTERS));
    HIPCHK_S(fc.sync());   // (the staging vectors leave scope below)
  }
  HIPCHK_S(fc.begin_span());
  if (replayed) sizes_and_filter(0xffffffffu, nullptr);
  scan(fc.ptr(s_keep), F, nullptr, fc.ptr(s_trank), cnt + TB_CAND_TRACKS);
  scan(fc.ptr(s_ksize), F, nullptr, fc.ptr(s_toff), cnt + TB_CAND_OBS);
  HIPCHK_S(fc.end_span());
  if (int st = read_counters()) return (gsfm_status)st;
  const size_t Tc = h_cnt[TB_CAND_TRACKS], C = h_cnt[TB_CAND_OBS];

  // ---- span 3: layout, order and duplicates per track, compaction --------------------------------------------------------------------
  if (Tc > 0) {
    HIPCHK_S(fc.begin_span());
    hipLaunchKernelGGL(k_tb_tracks, grid(F), blk, 0, s, n_feat, (const uint32_t*)fc.ptr(s_keep), (const uint32_t*)fc.ptr(s_ksize), (const uint32_t*)fc.ptr(s_trank),
                       (const uint32_t*)fc.ptr(s_toff), fc.ptr(s_cbase), fc.ptr(s_clen), fc.ptr(s_cursor), fc.ptr(s_list0), fc.ptr(s_list1), fc.ptr(s_list2), cnt);
    hipLaunchKernelGGL(k_tb_place, grid(F), blk, 0, s, n_feat, (const uint32_t*)label, (const uint32_t*)fc.ptr(s_keep), (const uint32_t*)fc.ptr(s_trank),
                       (const uint32_t*)fc.ptr(s_cbase), fc.ptr(s_cursor), fc.ptr(s_cand));
    auto order = [&](auto G, const uint32_t* list, const uint32_t* n_list, size_t most) {   // `most`: a host bound of the class's tracks
      constexpr int g = decltype(G)::value;
      hipLaunchKernelGGL(k_tb_order<g>, grid(most, g == 64 ? 1 : 256 / g), dim3(g == 64 ? 64 : 256), 0, s, list, n_list, (const uint32_t*)fc.ptr(s_cbase),
                         (const uint32_t*)fc.ptr(s_clen), (const uint32_t*)fc.ptr(s_cand), fep, eview, fc.ptr(s_sorted), fc.ptr(s_ok), fc.ptr(s_valid), cnt);
    };
    order(std::integral_constant<int, 64>(), fc.ptr(s_list2), cnt + TB_CLASS2, std::min(Tc, C / 65 + 1));
    order(std::integral_constant<int, 16>(), fc.ptr(s_list1), cnt + TB_CLASS1, std::min(Tc, C / 9 + 1));
    order(std::integral_constant<int, 4>(), fc.ptr(s_list0), cnt + TB_CLASS0, Tc);
    scan(fc.ptr(s_ok), C, nullptr, fc.ptr(s_dest), cnt + TB_OBS);
    scan(fc.ptr(s_valid), Tc, nullptr, fc.ptr(s_frank), cnt + TB_TRACKS);
    hipLaunchKernelGGL(k_tb_emit_obs, grid(C), blk, 0, s, (const uint32_t*)(cnt + TB_CAND_OBS), (const uint32_t*)fc.ptr(s_ok), (const uint32_t*)fc.ptr(s_dest),
                       (const uint32_t*)fc.ptr(s_sorted), fep, eview, xy, fc.ptr(s_oview), fc.ptr(s_oxy));
    hipLaunchKernelGGL(k_tb_emit_ptr, grid(Tc), blk, 0, s, (const uint32_t*)(cnt + TB_CAND_TRACKS), (const uint32_t*)fc.ptr(s_valid), (const uint32_t*)fc.ptr(s_frank),
                       (const uint32_t*)fc.ptr(s_cbase), (const uint32_t*)fc.ptr(s_dest), (const uint32_t*)cnt, fc.ptr(s_optr));
    HIPCHK_S(fc.end_span());
    if (int st = read_counters()) return (gsfm_status)st;
    const size_t T = h_cnt[TB_TRACKS], O = h_cnt[TB_OBS];
    if (T > 0) {
      HIPCHK_S(fc.download(track_ptr_out, s_optr, T + 1)); HIPCHK_S(fc.download(obs_view_out, s_oview, O)); HIPCHK_S(fc.download(obs_xy_out, s_oxy, O));
      HIPCHK_S(fc.sync());
    }
    *n_tracks = T; *n_obs = O;
  }
  if (kernel_ms) *kernel_ms = fc.kernel_ms();
  if (counts_out) {
    const uint64_t c[7] = {F, h_cnt[TB_COMPONENTS], h_cnt[TB_SMALL], h_cnt[TB_INCONSISTENT], h_cnt[TB_DEGENERATE], replayed, *n_tracks};
    std::memcpy(counts_out, c, sizeof(c));
  }
  return GSFM_OK;
}

}  // namespace
#endif
