// The host structure of the robust L1 + IRLS rotation estimator (rot_l1l2.hpp): the per-camera CSR of the directed entries of the view
// graph, the row lists of the two lane classes and the connectivity check.  Host vectors in, host vectors out, no HIP:
// tests/cpp/rot_l1l2_structure_test.cpp builds it with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// A row of up to this many entries is gathered by 8 lanes, a longer one by a whole wavefront (rot_l1l2_kernels.hpp)
constexpr uint32_t L1_SHORT_ROW = 32;

// Every edge e = (i, j) has two directed entries: one in row i (at pos_i[e]) and one in row j (at pos_j[e]).  nbr is the entry's
// neighbour, ent = 2 e + side its edge and its end (side 1: the row is the edge's j, where A^T has +1; side 0: the i end, -1).  Within a
// row the neighbours ascend, ties in edge order (pos_structure.hpp's order): a repeated pair has one entry per listing, a reversed
// listing its own sign.  short_rows / long_rows: the free cameras (an edge, not the fixed camera) by row length; the fixed camera has no
// column and is in neither.
struct L1Structure {
  std::vector<uint32_t> row_ptr, nbr, ent, pos_i, pos_j, short_rows, long_rows;
  std::vector<double> degree;     // per camera: its number of entries (the diagonal of the unweighted Laplacian); 1 on the others
  std::vector<uint8_t> present;   // per camera: it appears in an edge
  uint32_t n_present = 0;         // N
};

// (the camera indices are in range, no edge joins a camera to itself, fixed_cam is in range and 2 n_edges fits 32 bits: the caller has checked)
L1Structure l1_build_structure(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, uint32_t fixed_cam) {
  const size_t N = n_cams, E = n_edges, ND = 2 * E;
  L1Structure s;
  s.row_ptr.assign(N + 1, 0);
  for (size_t e = 0; e < E; ++e) { s.row_ptr[edge_i[e] + 1]++; s.row_ptr[edge_j[e] + 1]++; }
  for (size_t k = 0; k < N; ++k) s.row_ptr[k + 1] += s.row_ptr[k];
  std::vector<uint32_t> by_nbr(ND);   // u = 2 e + side, sorted by neighbour; then a stable sort by row
  {
    std::vector<uint32_t> fill(s.row_ptr.begin(), s.row_ptr.end() - 1);
    for (size_t e = 0; e < E; ++e) { by_nbr[fill[edge_j[e]]++] = (uint32_t)(2 * e); by_nbr[fill[edge_i[e]]++] = (uint32_t)(2 * e + 1); }
  }
  s.nbr.resize(ND); s.ent.resize(ND); s.pos_i.resize(E); s.pos_j.resize(E);
  {
    std::vector<uint32_t> fill(s.row_ptr.begin(), s.row_ptr.end() - 1);
    for (size_t t = 0; t < ND; ++t) {
      const uint32_t u = by_nbr[t], e = u >> 1, side = u & 1;
      const uint32_t row = side ? edge_j[e] : edge_i[e], m = side ? edge_i[e] : edge_j[e];
      const uint32_t d = fill[row]++;
      s.nbr[d] = m; s.ent[d] = u;
      (side ? s.pos_j : s.pos_i)[e] = d;
    }
  }
  s.present.resize(N); s.degree.resize(N);
  for (size_t k = 0; k < N; ++k) {
    const uint32_t len = s.row_ptr[k + 1] - s.row_ptr[k];
    s.present[k] = len > 0;
    s.n_present += len > 0;
    s.degree[k] = len > 0 ? (double)len : 1.0;
    if (len == 0 || k == fixed_cam) continue;
    (len <= L1_SHORT_ROW ? s.short_rows : s.long_rows).push_back((uint32_t)k);
  }
  return s;
}

// The first camera with an edge that no path joins to fixed_cam, or -1: union-find with path halving over the edges
int64_t l1_first_unreachable(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, uint32_t fixed_cam) {
  std::vector<uint32_t> parent(n_cams);
  for (uint32_t c = 0; c < n_cams; ++c) parent[c] = c;
  auto find = [&](uint32_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
  std::vector<uint8_t> has_edge(n_cams, 0);
  for (uint64_t e = 0; e < n_edges; ++e) {
    has_edge[edge_i[e]] = has_edge[edge_j[e]] = 1;
    const uint32_t a = find(edge_i[e]), b = find(edge_j[e]);
    if (a != b) parent[a < b ? b : a] = a < b ? a : b;
  }
  const uint32_t root = find(fixed_cam);
  for (uint32_t c = 0; c < n_cams; ++c)
    if (has_edge[c] && find(c) != root) return (int64_t)c;
  return -1;
}

}  // namespace
