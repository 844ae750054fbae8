// The host structure of a position problem (csrc/pos_structure.hpp), built by the host compiler alone: no HIP header, no device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "pos_structure.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

using U32 = std::vector<uint32_t>;

int main() {
  {
    // 5 cameras, camera 3 in no edge; 6 edges: (0, 1) twice (edges 0 and 3), the pair {2, 4} in both orientations (edges 1 and 4)
    const U32 ei = {0, 2, 1, 0, 4, 4}, ej = {1, 4, 2, 1, 2, 0};
    const PosStructure s = pos_build_structure(5, 6, ei.data(), ej.data());
    // rows: 0: (1 e0) (1 e3) (4 e5) | 1: (0 e0) (0 e3) (2 e2) | 2: (1 e2) (4 e1) (4 e4) | 3: -- | 4: (0 e5) (2 e1) (2 e4)
    CHECK((s.row_ptr == U32{0, 3, 6, 9, 9, 12}));
    CHECK((s.nbr == U32{1, 1, 4, 0, 0, 2, 1, 4, 4, 0, 2, 2}));
    CHECK((s.eid == U32{0, 3, 5, 0, 3, 2, 2, 1, 4, 5, 1, 4}));
    CHECK((s.pos_i == U32{0, 7, 5, 1, 11, 9}));
    CHECK((s.pos_j == U32{3, 10, 6, 4, 8, 2}));
    CHECK((s.present == std::vector<uint8_t>{1, 1, 1, 0, 1}));
  }
  {
    // 200 cameras (the last ten in no edge), 1500 random edges with many repeated pairs, against a plain sort of (row, neighbour, edge)
    const uint32_t N = 200, E = 1500;
    std::mt19937 rng(7);
    U32 ei(E), ej(E);
    for (uint32_t e = 0; e < E; ++e) {
      ei[e] = rng() % (N - 10);
      do ej[e] = rng() % (N - 10); while (ej[e] == ei[e]);
      if (e % 7 == 3) { ei[e] = ei[e - 1]; ej[e] = ej[e - 1]; }   // a repeated pair
      if (e % 7 == 5) { ei[e] = ej[e - 1]; ej[e] = ei[e - 1]; }   // ... and one the other way round
    }
    const PosStructure s = pos_build_structure(N, E, ei.data(), ej.data());
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> want;   // row, neighbour, edge, side
    for (uint32_t e = 0; e < E; ++e) { want.emplace_back(ei[e], ej[e], e, 0u); want.emplace_back(ej[e], ei[e], e, 1u); }
    std::sort(want.begin(), want.end());
    CHECK(s.row_ptr.size() == N + 1 && s.nbr.size() == 2 * E && s.eid.size() == 2 * E && s.pos_i.size() == E && s.pos_j.size() == E && s.present.size() == N);
    CHECK(s.row_ptr[0] == 0 && s.row_ptr[N] == 2 * E);
    std::vector<uint32_t> deg(N, 0);
    for (size_t d = 0; d < want.size(); ++d) {
      const auto [row, m, e, side] = want[d];
      deg[row]++;
      CHECK(s.row_ptr[row] <= d && d < s.row_ptr[row + 1]);
      CHECK(s.nbr[d] == m && s.eid[d] == e);
      CHECK((side ? s.pos_j : s.pos_i)[e] == d);
    }
    for (uint32_t k = 0; k < N; ++k) { CHECK(s.row_ptr[k + 1] - s.row_ptr[k] == deg[k]); CHECK(s.present[k] == (deg[k] > 0)); }
    for (uint32_t k = N - 10; k < N; ++k) CHECK(!s.present[k]);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("PASSED\n");
  return 0;
}
