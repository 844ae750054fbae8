// Host side, part 6a: the structure builders of gsfm_rot_problem_create that only read and write host vectors -- locality relabelling, connected
// components, block-CSR rows of the directed entries, cost tiles, the host half of the column-sorted layout.  What they fill (HostStructure,
// ColsortHost) is uploaded by problem_create.hpp.
#pragma once
#include "host_common.hpp"

namespace {

// Reverse Cuthill-McKee style relabelling (plain BFS from a minimum-degree camera of every component, reversed).  The p[col]
// and q[col] gathers of K3/K2 are bound by uncoalesced lane requests; when the neighbours of a camera sit within a few
// hundred indices of each other the lanes of a row share 128-byte lines and the gather becomes free (tools/archive/bench_matvec.hip:
// 346 us -> 235 us at a window of 400, 284 us at 2000, no gain at 20000).  View graphs of real scenes are spatially
// coherent but their ids are arbitrary; a uniformly random graph (the C5 benchmark) has nothing to recover.  The
// relabelling is therefore adopted only if it shrinks the mean |i - j| over the edges by more than half AND brings it
// under 1024 (neighbours within about +-2000); small problems (< 2048 cameras: everything is cache-resident) are left alone.
// GSFM_REORDER=0 disables it, =1 forces adoption.  Returns true when `perm` (external -> internal) must be applied.
template <typename AdjVec>
bool reorder_for_locality(uint32_t n_cams, uint64_t n_edges, const uint32_t* ei, const uint32_t* ej, const std::vector<uint32_t>& ptr,
                          const AdjVec& adj /* neighbour | role << 31 */, std::vector<uint32_t>* perm) {
  perm->clear();
  const char* env = getenv("GSFM_REORDER");
  const int mode = env ? atoi(env) : -1;  // -1 auto, 0 off, 1 force
  if (mode == 0 || (mode < 0 && n_cams < 2048)) return false;
  double before = 0.0;
  for (uint64_t e = 0; e < n_edges; ++e) before += std::fabs((double)ei[e] - (double)ej[e]);
  before /= (double)n_edges;
  if (mode < 0 && before < 256.0) return false;  // already local (a mean index distance of 256 ~ neighbours within +-500)
  std::vector<uint32_t> stamp(n_cams, 0xffffffffu);
  if (mode < 0) {
    // cheap pre-test: in a spatially coherent graph the two-hop neighbourhood of a camera stays small; in a uniformly random
    // one it floods the graph.  32 probes, each capped at n_cams / 8 cameras.
    const uint32_t cap = n_cams / 8;
    int flooded = 0;
    for (uint32_t s = 0; s < 32; ++s) {
      const uint32_t c0 = (uint32_t)(((uint64_t)s * n_cams) / 32);
      uint32_t seen = 0;
      for (uint32_t d = ptr[c0]; d < ptr[c0 + 1] && seen < cap; ++d) {
        const uint32_t c1 = adj[d] & 0x7fffffffu;
        for (uint32_t d2 = ptr[c1]; d2 < ptr[c1 + 1] && seen < cap; ++d2) {
          const uint32_t c2 = adj[d2] & 0x7fffffffu;
          if (stamp[c2] != s) { stamp[c2] = s; ++seen; }
        }
      }
      flooded += seen >= cap;
    }
    if (flooded > 16) return false;
  }
  std::vector<uint32_t> by_degree(n_cams);
  for (uint32_t c = 0; c < n_cams; ++c) by_degree[c] = c;
  std::stable_sort(by_degree.begin(), by_degree.end(), [&](uint32_t a, uint32_t b) { return ptr[a + 1] - ptr[a] < ptr[b + 1] - ptr[b]; });
  std::vector<uint32_t> order;
  order.reserve(n_cams);
  std::vector<uint8_t> seen(n_cams, 0);
  for (uint32_t s0 : by_degree) {
    if (seen[s0]) continue;
    seen[s0] = 1;
    size_t head = order.size();
    order.push_back(s0);
    while (head < order.size()) {
      const uint32_t c = order[head++];
      for (uint32_t d = ptr[c]; d < ptr[c + 1]; ++d) { const uint32_t m = adj[d] & 0x7fffffffu; if (!seen[m]) { seen[m] = 1; order.push_back(m); } }
    }
  }
  std::vector<uint32_t> p(n_cams);
  for (uint32_t k = 0; k < n_cams; ++k) p[order[k]] = n_cams - 1 - k;
  double after = 0.0;
  for (uint64_t e = 0; e < n_edges; ++e) after += std::fabs((double)p[ei[e]] - (double)p[ej[e]]);
  after /= (double)n_edges;
  if (mode < 0 && !(after < 0.5 * before && after < 1024.0)) return false;
  perm->swap(p);
  return true;
}

// connected components of the view graph among the cameras that have at least one edge
uint32_t count_components(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j) {
  UnionFind uf(n_cams);
  std::vector<uint8_t> touched(n_cams, 0);
  for (uint64_t e = 0; e < n_edges; ++e) { uf.unite(edge_i[e], edge_j[e]); touched[edge_i[e]] = touched[edge_j[e]] = 1; }
  uint32_t comps = 0;
  for (uint32_t c = 0; c < n_cams; ++c) if (touched[c] && uf.find(c) == c) ++comps;
  return comps;
}

// What the create phases build on the host before anything goes to the device.  The first block is the input (set once by the caller); the
// phases fill the rest in the order of the members.
struct HostStructure {
  uint32_t n_cams = 0, own_begin = 0, own_end = 0, n_rows = 0;   // rows = the cameras [own_begin, own_end) this process owns (all of them unsharded)
  bool sharded = false;
  uint64_t n_edges = 0;
  const uint32_t *edge_i = nullptr, *edge_j = nullptr;   // the caller's arrays, or ei_perm / ej_perm once a relabelling is adopted
  std::vector<uint32_t> ei_perm, ej_perm;
  std::vector<uint32_t> rp;      // build_rows: row pointers of the directed entries
  hvec<uint32_t> col, deid;      //   ... neighbour | role << 31 and edge of every entry (sized once, filled completely by the threads; the
                                 //   column-sorted layout REPLACES them by their position-ordered forms)
  std::vector<uint32_t> cost_eid;   // build_rows: the edges this process counts in the cost; build_cost_tiles: ordered by tile
  std::vector<CostTile> tiles;      // build_cost_tiles
  std::vector<uint2> cidx;          //   ... the two cameras of every cost edge, global or block-local
  size_t nd() const { return rp[n_rows]; }
};

// ---- directed entries by row (counting sort), cost-owned edges ----
int build_rows(HostStructure& H, int n_threads) {
  const uint32_t n_cams = H.n_cams, ob = H.own_begin, oe = H.own_end, *edge_i = H.edge_i, *edge_j = H.edge_j;
  const uint64_t n_edges = H.n_edges;
  auto owned = [&](uint32_t c) { return c >= ob && c < oe; };
  auto& rp = H.rp;
  auto& cost_eid = H.cost_eid;
  rp.assign((size_t)H.n_rows + 1, 0);
  cost_eid.clear();
  cost_eid.reserve(H.sharded ? n_edges / 2 + 16 : n_edges);
  if (!H.sharded && n_edges >= 200000 && n_threads > 1) {   // one GPU: every camera and every edge is owned; count on all threads
    std::vector<int> bad((size_t)n_threads, 0);
    parallel_run(n_threads, [&](int t, int T) {
      const uint64_t lo = n_edges * t / T, hi = n_edges * (t + 1) / T;
      for (uint64_t e = lo; e < hi; ++e) if (edge_i[e] >= n_cams || edge_j[e] >= n_cams || edge_i[e] == edge_j[e]) { bad[t] = 1; break; }
    });
    for (int b : bad) if (b) return fail(GSFM_ERR_INVALID_ARG, "edge with an out-of-range or repeated camera index");
    parallel_count(n_threads, 2 * n_edges, n_cams, [&](size_t u) { return (u & 1) ? edge_j[u >> 1] : edge_i[u >> 1]; }, rp.data() + 1);
    cost_eid.resize(n_edges);
    for (uint64_t e = 0; e < n_edges; ++e) cost_eid[e] = (uint32_t)e;
  } else
  for (uint64_t e = 0; e < n_edges; ++e) {
    const uint32_t i = edge_i[e], j = edge_j[e];
    if (i >= n_cams || j >= n_cams || i == j) return fail(GSFM_ERR_INVALID_ARG, "edge with an out-of-range or repeated camera index");
    if (owned(i)) rp[i - ob + 1]++;
    if (owned(j)) rp[j - ob + 1]++;
    // each edge is cost-owned by exactly one rank: the owner of `first` if (i + j) is even, else of `second`
    const uint32_t c = (((i + j) & 1u) == 0u) ? i : j;
    if (owned(c)) cost_eid.push_back((uint32_t)e);
    else if (!owned(i) && !owned(j)) return fail(GSFM_ERR_INVALID_ARG, "sharded problem: edge touches no owned camera");
  }
  for (size_t r = 0; r < H.n_rows; ++r) rp[r + 1] += rp[r];
  H.col.resize(rp[H.n_rows]); H.deid.resize(rp[H.n_rows]);
  // Fill: the random writes into col / deid (8 B per directed entry) are what costs.  An edge is two items, (first -> second) and
  // (second -> first, with the role bit), keyed by the row they go to; every row receives its entries in edge order.
  stable_scatter(n_edges >= 200000 ? n_threads : 1, 2 * n_edges, rp,
                 [&](size_t u) { return (uint32_t)(((u & 1) ? edge_j[u >> 1] : edge_i[u >> 1]) - ob); },
                 [&](size_t u, uint32_t d) { H.col[d] = (u & 1) ? (edge_i[u >> 1] | 0x80000000u) : edge_j[u >> 1]; H.deid[d] = (uint32_t)(u >> 1); });
  return 0;
}

// ---- optional locality relabelling of the cameras (unsharded: the rows are the full adjacency; see reorder_for_locality) ----
// Adopted: `perm` is filled, the edges and the rows are rebuilt in the new numbering and every row is ordered by neighbour.
int relabel_rows(HostStructure& H, std::vector<uint32_t>* perm, int n_threads) {
  if (H.sharded || !reorder_for_locality(H.n_cams, H.n_edges, H.edge_i, H.edge_j, H.rp, H.col, perm)) return 0;
  H.ei_perm.resize(H.n_edges); H.ej_perm.resize(H.n_edges);
  for (uint64_t e = 0; e < H.n_edges; ++e) { H.ei_perm[e] = (*perm)[H.edge_i[e]]; H.ej_perm[e] = (*perm)[H.edge_j[e]]; }
  H.edge_i = H.ei_perm.data(); H.edge_j = H.ej_perm.data();
  if (int st = build_rows(H, n_threads)) return st;
  // order every row by neighbour so that adjacent lanes gather adjacent cameras
  std::vector<std::pair<uint32_t, uint32_t>> row;
  for (size_t r = 0; r < H.n_rows; ++r) {
    row.clear();
    for (uint32_t d = H.rp[r]; d < H.rp[r + 1]; ++d) row.emplace_back(H.col[d], H.deid[d]);
    std::sort(row.begin(), row.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
      const uint32_t ca = a.first & 0x7fffffffu, cb = b.first & 0x7fffffffu;
      return ca != cb ? ca < cb : a.second < b.second;
    });
    for (uint32_t d = H.rp[r]; d < H.rp[r + 1]; ++d) { H.col[d] = row[d - H.rp[r]].first; H.deid[d] = row[d - H.rp[r]].second; }
  }
  return 0;
}

// Cost edges ordered by the tile (camera block of `first`, camera block of `second`), and by `first` inside a tile: two stable counting
// sorts, O(E + N + #tiles).  k_cost stages both blocks of a tile in LDS.  Fills tiles and cidx, reorders cost_eid; returns cost_direct.
bool build_cost_tiles(HostStructure& H, int n_threads) {
  const uint32_t n_cams = H.n_cams, *edge_i = H.edge_i, *edge_j = H.edge_j;
  auto& cost_eid = H.cost_eid;
  auto& tiles = H.tiles;
  const size_t Ec = cost_eid.size();
  const int T = Ec >= 200000 ? n_threads : 1;   // threads of the scatters
  std::vector<uint32_t> tmp(Ec), cnt((size_t)n_cams + 1, 0);
  parallel_count(n_threads, Ec, n_cams, [&](size_t u) { return edge_i[cost_eid[u]]; }, cnt.data() + 1);
  for (size_t c = 0; c < n_cams; ++c) cnt[c + 1] += cnt[c];
  stable_scatter(T, Ec, cnt, [&](size_t u) { return edge_i[cost_eid[u]]; }, [&](size_t u, uint32_t d) { tmp[d] = cost_eid[u]; });
  const uint64_t nblk = ((uint64_t)n_cams + GSFM_CAMBLOCK - 1) / GSFM_CAMBLOCK;
  auto tile_of = [&](uint32_t e) { return (uint64_t)(edge_i[e] / GSFM_CAMBLOCK) * nblk + edge_j[e] / GSFM_CAMBLOCK; };
  // The bucket table has nblk^2 entries: beyond 4096 camera blocks (8.4M cameras) the edges simply stay ordered by
  // `first` (such a sweep is far too thin for LDS tiles anyway).
  const bool bucketed = nblk <= 4096;
  std::vector<size_t> tstart(bucketed ? nblk * nblk + 1 : 1, 0);
  size_t populated = 0;
  if (bucketed) {
    {
      std::vector<uint32_t> tc(nblk * nblk + 1, 0);
      parallel_count(n_threads, Ec, nblk * nblk, [&](size_t u) { return tile_of(tmp[u]); }, tc.data() + 1);
      for (uint64_t b = 0; b < nblk * nblk; ++b) tstart[b + 1] = tstart[b] + tc[b + 1];
    }
    stable_scatter(T, Ec, tstart, [&](size_t u) { return tile_of(tmp[u]); }, [&](size_t u, size_t d) { cost_eid[d] = tmp[u]; });
    for (uint64_t b = 0; b < nblk * nblk; ++b) populated += tstart[b + 1] > tstart[b];
  } else {
    cost_eid = tmp;
  }
  // Thin tiles cannot amortise the 128 KiB LDS fill (88 B streamed per edge): below ~4096 edges per populated tile the
  // sweep gathers the quaternions directly instead (k_cost_direct).  GSFM_K1_DIRECT=0/1 overrides (A/B measurements).
  bool cost_direct = !bucketed || (populated > 0 && Ec / populated < 4096);
  if (const char* v = getenv("GSFM_K1_DIRECT")) cost_direct = !bucketed || atoi(v) != 0;
  if (cost_direct) {
    const size_t chunk = std::min<size_t>(8192, std::max<size_t>(GSFM_BLOCK, (Ec + 2047) / 2048));
    for (size_t lo = 0; lo < Ec; lo += chunk) tiles.push_back(CostTile{0, 0, (uint32_t)lo, (uint32_t)std::min(Ec, lo + chunk)});
  } else {
    // one workgroup per <= max_tile edges of a tile: ~2 workgroups per CU for big sweeps, >= 1 pass of 1024 lanes for small ones
    const size_t max_tile = std::min<size_t>(16384, std::max<size_t>(GSFM_TILE_THREADS, (Ec + 511) / 512));
    for (uint64_t b = 0; b < nblk * nblk; ++b) {
      size_t lo = tstart[b];
      const size_t hi = tstart[b + 1];
      while (lo < hi) {
        const size_t ce = std::min(hi, lo + max_tile);
        tiles.push_back(CostTile{(uint32_t)(b / nblk), (uint32_t)(b % nblk), (uint32_t)lo, (uint32_t)ce});
        lo = ce;
      }
    }
  }
  if (tiles.empty()) tiles.push_back(CostTile{0, 0, 0, 0});
  H.cidx.resize(Ec);
  const uint32_t idx_mod = cost_direct ? 0xffffffffu : (uint32_t)GSFM_CAMBLOCK;   // global or block-local camera indices
  parallel_run(T, [&](int t, int TT) {
    const size_t lo = Ec * t / TT, hi = Ec * (t + 1) / TT;
    for (size_t u = lo; u < hi; ++u)
      H.cidx[u] = cost_direct ? make_uint2(edge_i[cost_eid[u]], edge_j[cost_eid[u]]) : make_uint2(edge_i[cost_eid[u]] % idx_mod, edge_j[cost_eid[u]] % idx_mod);
  });
  return cost_direct;
}

// ---- host half of the column-sorted layout of the directed entries (colsort_kernels.hpp) ----
// Positions grouped by row block, sorted by column inside a block, cut into sub-chunks of GSFM_COL_SUB (each with its row-sorted slot
// permutation and per-row slot offsets), the sub-chunks of a block dealt to `nch` workgroups.
struct ColsortHost {
  uint32_t nch = 0, cbits = 0, cmax = 0;
  size_t n_pos = 0;
  hvec<uint32_t> col, eid, kcol;   // position-ordered col / deid (padding: GSFM_COL_PAD / edge 0); K3c's 4-byte record
  hvec<uint2> meta;
  hvec<uint16_t> kcnt;
  int k16_mode = -1;               // GSFM_K3C_K16: -1 auto, 0 the 2-byte record is not built, 1 forced
  hvec<uint16_t> k16;              // K3c's 2-byte record (ColLayoutDev::k16) with its per-wavefront bases and its escapes
  hvec<uint32_t> kbase, kdel;
  uint64_t k16_escapes = 0;
  std::vector<ColWg> wg;
};

// Workgroups per block (each writes one partial sum per row, which the finish kernels add): about 22 sub-chunks (11 k entries) per
// workgroup, but at least ~400 workgroups in all.  Measured on K3c + finish, same box each (profiles/r03_k3c_tuning.txt, r03_rank_share.txt):
// C5 on one GPU (196 blocks of ~200 sub-chunks) 8 / 9 / 10 per block = 208 / 202 / 203 us; one rank of 4 (49 blocks) 8 / 13 / 17 / 32 =
// 51 / 57 / 61 / 64 us; one rank of 8 (25 blocks) 8 / 16 / 24 / 32 = 39.5 / 33.3 / 38 / 39 us.  GSFM_COL_WGS=n asks for n workgroups in all.
uint32_t colsort_workgroups_per_block(size_t n_sub, uint32_t nblk) {
  const double per_block = (double)n_sub / nblk;
  uint32_t nch = std::max<uint32_t>((uint32_t)std::lround(per_block / 22.0), (400 + nblk - 1) / nblk);
  // A layout that is ONE round of workgroups (fewer than the 1280 tasks from which the sizes are graded: a rank's share of a sharded problem, a
  // mid-size graph) runs as long as its most loaded CU: about two workgroups per CU -- 500 tasks -- measured best for K3c AND K2c on the
  // shares of the benchmark graph (profiles/r05_rank_wgs.txt: 2 ranks 882 -> 490 tasks K3c 106.6 -> 86.2 us; 8 ranks 400 -> 500 tasks K2c
  // 114.1 -> 104.6 us, K3c 34.6 -> 33.9; 525 or 750 tasks lose 15 %: a third workgroup on some CUs).
  if ((size_t)nblk * nch < 1280) nch = std::max<uint32_t>(1u, (uint32_t)std::lround(500.0 / nblk));
  if (const char* e = getenv("GSFM_COL_WGS")) { const int v = atoi(e); if (v > 0) nch = ((uint32_t)v + nblk - 1) / nblk; }
  return std::min<uint32_t>(32, std::max<uint32_t>(1, nch));
}

// The 2-byte record of one sub-chunk (positions base .. base + SUB, wavefront bases from kbase_at): cameras as steps inside each
// wavefront's 64 positions.  Returns the escapes: a step of GSFM_K16_DEL_ESC cameras or more, a row count of GSFM_K16_CNT_ESC or more.
uint32_t colsort_k16_subchunk(ColsortHost& L, size_t base, size_t kbase_at) {
  uint32_t prev = 0, esc = 0;
  for (uint32_t p = 0; p < GSFM_COL_SUB; ++p) {
    const size_t o = base + p;
    const uint32_t cam = L.meta[o].x == GSFM_COL_PAD ? prev : (L.meta[o].x & 0x7fffffffu);   // (position 0 of a sub-chunk is never padding)
    uint32_t step = 0;
    if ((p & 63u) == 0) L.kbase[kbase_at + (p >> 6)] = cam; else step = cam - prev;
    prev = cam;
    const uint32_t rc = L.kcnt[o];
    L.kdel[o] = step;
    esc += (step >= GSFM_K16_DEL_ESC) + (rc >= GSFM_K16_CNT_ESC);
    L.k16[o] = (uint16_t)(col_slot(L.meta[o].y) | (std::min(rc, GSFM_K16_CNT_ESC) << GSFM_COL_SLOT_BITS) | (std::min(step, GSFM_K16_DEL_ESC) << 12));
  }
  return esc;
}

// Host, once per problem, blocks in parallel.  In: the row-major CSR (rp, col with the role bit, deid = edge of every entry).  Returns false
// where the layout does not apply (no rows, too many cameras or positions for the packed words): the problem stays on the row-major form.
bool build_colsort_host(uint32_t n_cams, uint32_t n_rows, const std::vector<uint32_t>& rp, const hvec<uint32_t>& col, const hvec<uint32_t>& deid,
                        int n_threads, ColsortHost& L) {
  constexpr uint32_t RB = GSFM_COL_RB, SUB = GSFM_COL_SUB;
  const uint32_t nblk = (n_rows + RB - 1) / RB;
  if (nblk == 0 || n_cams >= (1u << (31 - GSFM_COL_SLOT_BITS)) - 1u) return false;   // (camera | slot | count in one 32-bit word: 2^22 cameras at 512 rows per block)
  uint32_t cbits = 1;
  while (((1u << cbits) - 1u) <= n_cams) ++cbits;   // cameras 0 .. n_cams - 1 and the all-ones padding value
  const uint32_t cmax = cbits + GSFM_COL_SLOT_BITS <= 28 ? (1u << (32 - GSFM_COL_SLOT_BITS - cbits)) - 1u : 0u, kpad = (1u << cbits) - 1u;   // (RB = 512: counts up to 2^(23 - cbits) - 1 in the word, as before)
  std::vector<size_t> sub_off((size_t)nblk + 1, 0);
  for (uint32_t b = 0; b < nblk; ++b) {
    const size_t ne = rp[std::min(n_rows, (b + 1) * RB)] - rp[b * RB];
    sub_off[b + 1] = sub_off[b] + (ne + SUB - 1) / SUB;
  }
  const size_t n_sub = sub_off[nblk], n_pos = n_sub * SUB;
  const uint32_t nch = colsort_workgroups_per_block(n_sub, nblk);
  if (n_pos == 0 || n_pos >= 0x7fffffffull) return false;   // (positions are 32-bit in the kernels: stay on the row-major form)
  L.nch = nch; L.cbits = cbits; L.cmax = cmax; L.n_pos = n_pos;
  L.col.resize(n_pos); L.eid.resize(n_pos); L.kcol.resize(n_pos);   // (every position is written below)
  L.meta.resize(n_pos);
  L.kcnt.resize(n_pos);
  // K3c's 2-byte record (ColLayoutDev::k16): GSFM_K3C_K16=0 keeps the 4-byte one (A/B), =1 forces it whatever its escapes cost
  const char* k16_env = getenv("GSFM_K3C_K16");
  L.k16_mode = k16_env && *k16_env ? atoi(k16_env) : -1;
  if (L.k16_mode != 0) { L.k16.resize(n_pos); L.kbase.resize(n_sub * (SUB / 64)); L.kdel.resize(n_pos); }
  std::atomic<uint64_t> k16_escapes{0};
  L.wg.resize((size_t)nblk * nch);
  // (graded only where the tasks outnumber the chip's resident workgroups several times over -- K2c holds 512, K3c 1024 (four workgroups per CU
  // at its 37 vector registers; it held 768, three per CU, as long as its slot loop was unrolled to 74 registers): with a single round,
  // as on one rank's share of a sharded problem (400 tasks), the kernel takes as long as its LARGEST task, and grading made K3c 33 -> 40 us there)
  const bool graded = nch > 1 && (size_t)nblk * nch >= (size_t)1280;
  parallel_run(std::max(1, std::min<int>(n_threads, (int)nblk)), [&](int t, int T) {
    std::vector<std::pair<uint64_t, uint32_t>> ent;   // (camera << 16 | local row, d): a repeated camera pair is ordered by d
    std::vector<uint32_t> cnt(RB + 1), fill(RB), chist;
    for (uint32_t b = (uint32_t)t; b < nblk; b += (uint32_t)T) {
      const uint32_t r0 = b * RB, r1 = std::min(n_rows, r0 + RB);
      const size_t ne = rp[r1] - rp[r0], ns = sub_off[b + 1] - sub_off[b];
      if ((size_t)n_cams <= 4 * ne + 4096) {
        // counting sort by camera: the rows are walked in order and a row's entries are in edge order, so equal cameras keep (row, d) order --
        // the same sequence as sorting the (camera, row, d) triples (199 -> ... ms of the 100k / 10M problem's creation)
        chist.assign((size_t)n_cams + 1, 0u);
        for (uint32_t d = rp[r0]; d < rp[r1]; ++d) chist[(col[d] & 0x7fffffffu) + 1]++;
        for (uint32_t c = 0; c < n_cams; ++c) chist[c + 1] += chist[c];
        ent.resize(ne);
        for (uint32_t r = r0; r < r1; ++r) for (uint32_t d = rp[r]; d < rp[r + 1]; ++d) {
          const uint32_t c = col[d] & 0x7fffffffu;
          ent[chist[c]++] = std::make_pair(((uint64_t)c << 16) | (r - r0), d);
        }
      } else {   // (a block far sparser than the camera range: forced layouts of small tests)
        ent.clear();
        for (uint32_t r = r0; r < r1; ++r) for (uint32_t d = rp[r]; d < rp[r + 1]; ++d) ent.emplace_back(((uint64_t)(col[d] & 0x7fffffffu) << 16) | (r - r0), d);
        std::sort(ent.begin(), ent.end());
      }
      // The tasks of a block: its sub-chunks cut into nch ranges of DECREASING size (1.5 x the mean down to 0.5 x), launched chunk-major --
      // the large tasks of all blocks first, the small ones last.  Equal tasks fill the chip in whole rounds (K2c: 2 x 256 resident
      // workgroups, 1764 equal tasks = 3.45 rounds, the last one half empty; measured as a saw-tooth in the task count: 616 us at 1960
      // tasks, 645 at 2156, 612 at 2548: profiles/r04b_wgs_sweep.txt); with graded sizes the tail is as long as the SMALLEST task.
      for (uint32_t c = 0; c < nch; ++c) {
        size_t lo, hi;
        if (graded && ns >= 4 * (size_t)nch) {
          // cumulative weight of chunks 0 .. c-1 with w_c = 1.5 - c / (nch - 1), total nch
          auto cum = [&](uint32_t k) { return 1.5 * k - 0.5 * (double)k * (k - 1) / (double)(nch - 1); };
          lo = (size_t)std::llround((double)ns * cum(c) / (double)nch); hi = (size_t)std::llround((double)ns * cum(c + 1) / (double)nch);
          if (c + 1 == nch) hi = ns;
        } else { lo = ns * c / nch; hi = ns * (c + 1) / nch; }
        L.wg[(size_t)c * nblk + b] = ColWg{(uint32_t)(sub_off[b] + lo), (uint32_t)(hi - lo), r0, b * nch + c};
      }
      for (size_t s = 0; s < ns; ++s) {
        const size_t lo = s * SUB, hi = std::min(ne, lo + SUB), base = (sub_off[b] + s) * SUB;
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (size_t e = lo; e < hi; ++e) cnt[(ent[e].first & 0xffff) + 1]++;
        for (uint32_t r = 0; r < RB; ++r) cnt[r + 1] += cnt[r];
        std::copy(cnt.begin(), cnt.end() - 1, fill.begin());
        uint32_t pad_slot = (uint32_t)(hi - lo);
        for (size_t e = lo; e < lo + SUB; ++e) {
          const size_t o = base + (e - lo);
          const uint32_t p = (uint32_t)(e - lo), rc = cnt[p + 1] - cnt[p];   // position p also carries the slot count of ROW p
          if (e < hi) {
            const uint32_t rl = (uint32_t)(ent[e].first & 0xffff), d = ent[e].second;
            L.col[o] = col[d]; L.eid[o] = deid[d]; L.meta[o] = make_uint2(col[d], col_pack(fill[rl]++, rc, rl));
          } else { L.col[o] = GSFM_COL_PAD; L.eid[o] = 0; L.meta[o] = make_uint2(GSFM_COL_PAD, col_pack(pad_slot++, rc, 0)); }   // zero block, a slot no row reads
          L.kcol[o] = (L.meta[o].x == GSFM_COL_PAD ? kpad : (L.meta[o].x & 0x7fffffffu)) | (col_slot(L.meta[o].y) << cbits) | (std::min(rc, cmax) << (cbits + GSFM_COL_SLOT_BITS));
          L.kcnt[o] = (uint16_t)rc;
        }
        // the same sub-chunk once more for the 2-byte record
        if (L.k16_mode != 0) k16_escapes.fetch_add(colsort_k16_subchunk(L, base, (sub_off[b] + s) * (SUB / 64)), std::memory_order_relaxed);
      }
    }
  });
  L.k16_escapes = k16_escapes.load();
  return true;
}

}  // namespace
