// The component rest rule (globalsfmpy_amd/csrc/comp_rest.hpp) on a table of cases, built by the host compiler alone.
// Prints one line per failing case and "PASSED" when all hold.
#include <cmath>
#include <cstdio>
#include <limits>

#include "comp_rest.hpp"

namespace {

struct Case {
  const char* what;
  double cur, rad_cur, prev, rad_prev, freeze_below;
  bool rest;
};

const double INF = std::numeric_limits<double>::infinity();
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double FB = 1e-10;   // the threshold of the smooth losses (solver_pcg.hpp, comp_freeze_below)

const Case kCases[] = {
    // a damping-limited step scales with the radius: rejections at radius / 2, / 4, / 8 shrink it, and that proves nothing
    {"rejection: radius / 2", 4e-11, 5e2, 8e-11, 1e3, FB, false},
    {"rejection: radius / 4", 2e-11, 2.5e2, 4e-11, 5e2, FB, false},
    {"rejection: radius / 8", 1e-11, 1.25e2, 2e-11, 2.5e2, FB, false},
    {"rejections below a weak start", 5e-11, 1.25e3, 1e-10, 2.5e3, FB, false},
    // a tiny initial radius: the damping makes every step tiny, however long it stays at that radius
    {"tiny caller radius, first measurement", 5e-11, 1e-5, INF, 0.0, FB, false},
    {"tiny caller radius, step unchanged", 5e-11, 1e-5, 5e-11, 1e-5, FB, false},
    {"tiny caller radius, step grows with the radius", 9e-11, 3e-5, 5e-11, 1e-5, FB, false},
    // genuine contraction at an unchanged or growing radius
    {"contraction at the same radius", 4e-11, 1e2, 1e-9, 1e2, FB, true},
    {"contraction at a growing radius", 4e-11, 3e2, 1e-9, 1e2, FB, true},
    {"halved exactly at the same radius", 5e-11, 1e-3, 1e-10, 1e-3, FB, true},
    {"less than halved at the same radius", 6e-11, 1e-3, 1e-10, 1e-3, FB, false},
    // weak damping: the step is the Newton step
    {"weak damping, first measurement", 5e-11, 1e4, INF, 0.0, FB, true},
    {"weak damping after a rejection", 5e-11, 1e4, 1e-11, 2e4, FB, true},
    {"weak damping, large radius", 1e-10, 1e16, 1e-10, 1e16, FB, true},
    {"weak damping, step above the threshold", 2e-10, 1e8, 1e-9, 1e8, FB, false},
    // nothing measured: idle, failed factorisation (NaN or inf in the factor), start of a solve
    {"nothing measured (+inf)", INF, 1e4, 1e-9, 1e4, FB, false},
    {"NaN step", NaN, 1e4, 1e-9, 1e4, FB, false},
    {"NaN step at a growing radius", NaN, 2e2, 1e-9, 1e2, FB, false},
    {"previous measurement NaN", 1e-11, 1e2, NaN, 1e2, FB, false},
    // the MAGSAC losses: never
    {"MAGSAC, weak damping", 1e-14, 1e8, 1e-9, 1e8, 0.0, false},
    {"MAGSAC, contraction", 0.0, 1e2, 1e-9, 1e2, 0.0, false},
};

}  // namespace

int main() {
  int failed = 0;
  for (const Case& c : kCases) {
    const bool got = gsfm::comp_may_rest(c.cur, c.rad_cur, c.prev, c.rad_prev, c.freeze_below);
    if (got != c.rest) {
      std::printf("FAILED: %s: comp_may_rest(%g, %g, %g, %g, %g) = %d, expected %d\n", c.what, c.cur, c.rad_cur, c.prev, c.rad_prev, c.freeze_below, got, c.rest);
      ++failed;
    }
  }
  std::printf("%d cases, %d failed\n", (int)(sizeof(kCases) / sizeof(kCases[0])), failed);
  if (failed) return 1;
  std::printf("PASSED\n");
  return 0;
}
