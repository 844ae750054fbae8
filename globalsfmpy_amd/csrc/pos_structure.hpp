// The host structure of a position problem (solver_pos.hpp): the CSR of the directed entries of the view graph.  Host vectors in, host
// vectors out, no HIP: tests/cpp/pos_structure_test.cpp builds it with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// Every edge e = (i, j) has two directed entries: one in row i with neighbour j (at pos_i[e]) and one in row j with neighbour i (at
// pos_j[e]); nbr / eid are the neighbour and the edge of every entry.  Within a row the neighbours ascend, ties in edge order.
struct PosStructure {
  std::vector<uint32_t> row_ptr, nbr, eid, pos_i, pos_j;
  std::vector<uint8_t> present;   // per camera: it appears in an edge
};

// (the camera indices are in range and 2 n_edges fits 32 bits: the caller has checked)
PosStructure pos_build_structure(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j) {
  const size_t N = n_cams, E = n_edges, ND = 2 * E;
  PosStructure s;
  // counting sort by neighbour, then a stable one by row -> neighbours sorted within a row, ties in edge order
  s.row_ptr.assign(N + 1, 0);
  for (size_t e = 0; e < E; ++e) { s.row_ptr[edge_i[e] + 1]++; s.row_ptr[edge_j[e] + 1]++; }
  for (size_t k = 0; k < N; ++k) s.row_ptr[k + 1] += s.row_ptr[k];
  std::vector<uint32_t> by_nbr(ND);   // directed entry id u = 2 e + side (side 1: the j-end's entry), sorted by neighbour
  {
    std::vector<uint32_t> fill(s.row_ptr.begin(), s.row_ptr.end() - 1);
    for (size_t e = 0; e < E; ++e) { by_nbr[fill[edge_j[e]]++] = (uint32_t)(2 * e); by_nbr[fill[edge_i[e]]++] = (uint32_t)(2 * e + 1); }
  }
  s.nbr.resize(ND); s.eid.resize(ND); s.pos_i.resize(E); s.pos_j.resize(E);
  {
    std::vector<uint32_t> fill(s.row_ptr.begin(), s.row_ptr.end() - 1);
    for (size_t t = 0; t < ND; ++t) {
      const uint32_t u = by_nbr[t], e = u >> 1, side = u & 1;
      const uint32_t row = side ? edge_j[e] : edge_i[e], m = side ? edge_i[e] : edge_j[e];
      const uint32_t d = fill[row]++;
      s.nbr[d] = m; s.eid[d] = e;
      (side ? s.pos_j : s.pos_i)[e] = d;
    }
  }
  s.present.resize(N);
  for (size_t k = 0; k < N; ++k) s.present[k] = s.row_ptr[k + 1] > s.row_ptr[k];
  return s;
}

}  // namespace
