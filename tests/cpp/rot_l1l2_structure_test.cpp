// Host-compiler test of csrc/rot_l1l2_structure.hpp: the CSR of directed entries with its signs, duplicates and reversed listings, the
// lane classes with a hub, the fixed camera's row, and the connectivity check.  Built and run by tests/test_rot_l1l2_structure.py.
#include <algorithm>
#include <cstdio>
#include <random>

#include "rot_l1l2_structure.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// every property of the structure that a kernel relies on, against the edge list itself
static void check_against_edges(uint32_t N, const std::vector<uint32_t>& ei, const std::vector<uint32_t>& ej, uint32_t fixed) {
  const size_t E = ei.size();
  const L1Structure s = l1_build_structure(N, E, ei.data(), ej.data(), fixed);
  CHECK(s.row_ptr.size() == N + 1 && s.row_ptr[0] == 0 && s.row_ptr[N] == 2 * E);
  CHECK(s.nbr.size() == 2 * E && s.ent.size() == 2 * E && s.pos_i.size() == E && s.pos_j.size() == E);
  std::vector<int> seen(2 * E, 0);
  uint32_t present = 0;
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t beg = s.row_ptr[k], end = s.row_ptr[k + 1];
    CHECK(s.present[k] == (end > beg));
    present += end > beg;
    CHECK(s.degree[k] == (end > beg ? (double)(end - beg) : 1.0));
    for (uint32_t d = beg; d < end; ++d) {
      const uint32_t e = s.ent[d] >> 1, side = s.ent[d] & 1;
      CHECK(e < E);
      CHECK((side ? ej[e] : ei[e]) == k);          // side 1: the row is the edge's j end (+1 in A^T)
      CHECK(s.nbr[d] == (side ? ei[e] : ej[e]));
      CHECK((side ? s.pos_j[e] : s.pos_i[e]) == d);
      seen[s.ent[d]]++;
      if (d > beg) CHECK(s.nbr[d - 1] < s.nbr[d] || (s.nbr[d - 1] == s.nbr[d] && (s.ent[d - 1] >> 1) < e));   // neighbours ascend, ties in edge order
    }
  }
  for (int c : seen) CHECK(c == 1);
  CHECK(s.n_present == present);
  // the lane classes: every free camera exactly once, by row length; the fixed camera and cameras without an edge in neither
  std::vector<int> listed(N, 0);
  for (uint32_t k : s.short_rows) { CHECK(s.row_ptr[k + 1] - s.row_ptr[k] <= L1_SHORT_ROW); listed[k]++; }
  for (uint32_t k : s.long_rows) { CHECK(s.row_ptr[k + 1] - s.row_ptr[k] > L1_SHORT_ROW); listed[k]++; }
  for (uint32_t k = 0; k < N; ++k) CHECK(listed[k] == (s.present[k] && k != fixed ? 1 : 0));
  CHECK(std::is_sorted(s.short_rows.begin(), s.short_rows.end()) && std::is_sorted(s.long_rows.begin(), s.long_rows.end()));
}

int main() {
  {  // literals: 5 cameras (camera 3 without an edge), a pair listed twice, a pair in both orientations, a reversed listing
    const std::vector<uint32_t> ei = {0, 2, 0, 1, 4, 2}, ej = {1, 0, 1, 0, 2, 4};
    const L1Structure s = l1_build_structure(5, 6, ei.data(), ej.data(), 0);
    const std::vector<uint32_t> row_ptr = {0, 4, 7, 10, 10, 12};
    CHECK(s.row_ptr == row_ptr);
    // row 0: neighbours 1 (edges 0, 2, 3), 2 (edge 1); it is i of edges 0 and 2 (side 0), j of edges 3 and 1 (side 1)
    const std::vector<uint32_t> nbr0 = {1, 1, 1, 2}, ent0 = {0, 4, 7, 3};
    CHECK(std::equal(nbr0.begin(), nbr0.end(), s.nbr.begin()) && std::equal(ent0.begin(), ent0.end(), s.ent.begin()));
    // row 2: neighbours 0 (edge 1, i end), 4 (edge 4 as j, edge 5 as i)
    const std::vector<uint32_t> nbr2 = {0, 4, 4}, ent2 = {2, 9, 10};
    CHECK(std::equal(nbr2.begin(), nbr2.end(), s.nbr.begin() + 7) && std::equal(ent2.begin(), ent2.end(), s.ent.begin() + 7));
    CHECK(s.n_present == 4 && !s.present[3] && s.degree[3] == 1.0 && s.degree[0] == 4.0);
    const std::vector<uint32_t> free_rows = {1, 2, 4};   // the fixed camera's row is in no list
    CHECK(s.short_rows == free_rows && s.long_rows.empty());
    check_against_edges(5, ei, ej, 0);
    check_against_edges(5, ei, ej, 4);
    CHECK(l1_first_unreachable(5, 6, ei.data(), ej.data(), 0) == -1);   // camera 3 has no edge: not a parameter, not missed
  }
  {  // a hub joined to 299 cameras plus a ring: one long row; fixed at the hub and at a leaf
    std::vector<uint32_t> ei, ej;
    for (uint32_t k = 1; k < 300; ++k) { ei.push_back(0); ej.push_back(k); }
    for (uint32_t k = 1; k < 300; ++k) { ei.push_back(k % 299 + 1); ej.push_back(k); }   // (larger first, but for the last)
    const L1Structure hub_fixed = l1_build_structure(300, ei.size(), ei.data(), ej.data(), 0);
    CHECK(hub_fixed.long_rows.empty() && hub_fixed.short_rows.size() == 299);
    const L1Structure leaf_fixed = l1_build_structure(300, ei.size(), ei.data(), ej.data(), 5);
    CHECK(leaf_fixed.long_rows == std::vector<uint32_t>{0} && leaf_fixed.short_rows.size() == 298 && leaf_fixed.degree[0] == 299.0);
    check_against_edges(300, ei, ej, 0);
    check_against_edges(300, ei, ej, 5);
  }
  {  // rows of exactly L1_SHORT_ROW and L1_SHORT_ROW + 1 entries fall on either side of the threshold
    std::vector<uint32_t> ei, ej;
    for (uint32_t k = 0; k < L1_SHORT_ROW; ++k) { ei.push_back(0); ej.push_back(2 + k); }
    for (uint32_t k = 0; k < L1_SHORT_ROW + 1; ++k) { ei.push_back(2 + k); ej.push_back(1); }
    const uint32_t N = 3 + L1_SHORT_ROW;
    const L1Structure s = l1_build_structure(N, ei.size(), ei.data(), ej.data(), 2);
    CHECK(s.long_rows == std::vector<uint32_t>{1} && std::find(s.short_rows.begin(), s.short_rows.end(), 0u) != s.short_rows.end());
    check_against_edges(N, ei, ej, 2);
  }
  {  // a random multigraph with reversed and repeated pairs
    std::mt19937 rng(7);
    std::vector<uint32_t> ei, ej;
    for (int e = 0; e < 1500; ++e) {
      uint32_t a = rng() % 200, b = rng() % 200;
      if (a == b) b = (a + 1) % 200;
      ei.push_back(a); ej.push_back(b);
      if (e % 10 == 0) { ei.push_back(b); ej.push_back(a); }
      if (e % 15 == 0) { ei.push_back(a); ej.push_back(b); }
    }
    check_against_edges(200, ei, ej, 17);
  }
  {  // connectivity: two components, then joined
    std::vector<uint32_t> ei = {0, 1, 4, 5}, ej = {1, 2, 5, 6};
    CHECK(l1_first_unreachable(8, 4, ei.data(), ej.data(), 0) == 4);
    CHECK(l1_first_unreachable(8, 4, ei.data(), ej.data(), 6) == 0);
    ei.push_back(6); ej.push_back(2);
    CHECK(l1_first_unreachable(8, 5, ei.data(), ej.data(), 0) == -1);
  }
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
