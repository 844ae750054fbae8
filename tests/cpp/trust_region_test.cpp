// The host trust-region rule (csrc/trust_region.hpp), built by the host compiler alone.  Without arguments: five consecutive invalid steps.
// With "replay <initial radius> <max radius>": reads one step per line from stdin -- "I" (invalid), "R" (rejected) or "A <relative decrease>"
// (accepted), the numbers as hex floats -- and prints the radius after every step as the hex pattern of its 64 bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "trust_region.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "replay") == 0) {
    TrustRegion tr;
    tr.radius = std::strtod(argv[2], nullptr);
    const double max_radius = std::strtod(argv[3], nullptr);
    char line[128];
    while (std::fgets(line, sizeof(line), stdin)) {
      if (line[0] == 'I') { if (tr.invalid_step()) { std::printf("failed\n"); continue; } }
      else if (line[0] == 'R') { tr.num_invalid = 0; tr.rejected(); }
      else if (line[0] == 'A') { tr.num_invalid = 0; tr.accepted(std::strtod(line + 1, nullptr), max_radius); }
      else continue;
      std::printf("%016llx\n", bits(tr.radius));
    }
    return 0;
  }
  {
    // HandleInvalidStep five times in a row: the radius shrinks by 2, 4, 8, 16, the fifth ends the solve and leaves the state alone
    TrustRegion tr;
    tr.radius = 1e4;
    const double want[4] = {1e4 / 2, 1e4 / 2 / 4, 1e4 / 2 / 4 / 8, 1e4 / 2 / 4 / 8 / 16};
    for (int k = 0; k < 4; ++k) { CHECK(!tr.invalid_step()); CHECK(tr.radius == want[k]); CHECK(tr.num_invalid == k + 1); }
    CHECK(tr.decrease_factor == 32.0);
    CHECK(tr.invalid_step());
    CHECK(tr.radius == want[3] && tr.decrease_factor == 32.0);
  }
  {
    // a valid step in between starts the count again; an accepted one resets the decrease factor, a rejected one does not
    TrustRegion tr;
    tr.radius = 1.0;
    for (int k = 0; k < 4; ++k) CHECK(!tr.invalid_step());
    tr.num_invalid = 0;
    tr.rejected();
    CHECK(tr.radius == 1.0 / 1024 / 32 && tr.decrease_factor == 64.0);
    for (int k = 0; k < 4; ++k) CHECK(!tr.invalid_step());
    tr.num_invalid = 0;
    tr.accepted(1.0, 1e16);   // 1 - (2 - 1)^3 = 0: the 3 x clamp
    CHECK(tr.decrease_factor == 2.0);
    tr.radius = 1e16;
    tr.accepted(1.0, 1e16);
    CHECK(tr.radius == 1e16);   // capped at the maximum
    tr.radius = 8.0;
    tr.accepted(0.5, 1e16);     // 1 - 0^3 = 1: unchanged
    CHECK(tr.radius == 8.0);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("PASSED\n");
  return 0;
}
