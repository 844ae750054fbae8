// The slab layout of the one-shot device calls (csrc/flat_call.hpp, FlatLayout), built by the host compiler alone: no HIP header, no device.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "flat_call.hpp"

struct double4 { double x, y, z, w; };   // (the device type's size and nothing else)

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static size_t up(size_t b) { return (b + 255) / 256 * 256; }

int main() {
  {
    // The take list of trans_refine_impl for E = 3 edges, N = 2 cameras, M = 5 matches, against the offsets of the hand-written
    // cursor it replaces (bytes 4E 4E 4E 8(E+1) 32M 48E 24N 24E 24M 24E 4E 4E 8E = 12 12 12 32 160 144 48 72 120 72 12 12 24,
    // each below 256: one 256-byte step per array).
    const size_t E = 3, N = 2, M = 5;
    FlatLayout L;
    const size_t got[] = {L.take<uint32_t>(E).off, L.take<uint32_t>(E).off, L.take<uint32_t>(E).off, L.take<uint64_t>(E + 1).off, L.take<double4>(M).off,
                          L.take<double>(6 * E).off, L.take<double>(3 * N).off, L.take<double>(3 * E).off, L.take<double>(3 * M).off,
                          L.take<double>(3 * E).off, L.take<int32_t>(E).off, L.take<int32_t>(E).off, L.take<double>(E).off};
    const size_t want[] = {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072};
    for (int k = 0; k < 13; ++k) CHECK(got[k] == want[k]);
    CHECK(L.total == 3328);
  }
  {
    // Sizes around the 256-byte step, zero counts first, in the middle, repeated and last, several element sizes.
    struct Take { size_t elem, count; };
    const std::vector<Take> takes = {{4, 0}, {1, 1}, {1, 255}, {1, 256}, {1, 257}, {8, 0}, {8, 0}, {8, 32}, {8, 33}, {4, 1000}, {32, 8}, {32, 9},
                                     {16, 12345}, {2, 0}, {8, 1}, {4, 0}};
    FlatLayout L;
    std::vector<size_t> off;
    for (const Take& t : takes) {
      const size_t before = L.total;
      size_t o = 0;
      switch (t.elem) {
        case 1: o = L.take<uint8_t>(t.count).off; break;
        case 2: o = L.take<uint16_t>(t.count).off; break;
        case 4: o = L.take<uint32_t>(t.count).off; break;
        case 8: o = L.take<double>(t.count).off; break;
        case 16: o = L.take<long double>(t.count).off; break;
        default: o = L.take<double4>(t.count).off; break;
      }
      CHECK(o == before);                                   // take order: a slot starts where the one before it ended
      CHECK(o % 256 == 0);
      CHECK(L.total == o + up(t.elem * t.count));           // the total is the last offset plus its rounded size
      if (t.count == 0) CHECK(L.total == before);           // a zero-count take consumes nothing
      else CHECK(L.total >= o + t.elem * t.count && L.total - (o + t.elem * t.count) < 256);   // room for the array, less than a step to spare
      off.push_back(o);
    }
    for (size_t k = 0; k + 1 < takes.size(); ++k) CHECK(off[k] + takes[k].elem * takes[k].count <= off[k + 1]);   // slots do not overlap
    CHECK(L.total % 256 == 0);
  }
  static_assert(sizeof(long double) == 16 && sizeof(double4) == 32, "the table's element sizes");
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("PASSED\n");
  return 0;
}
