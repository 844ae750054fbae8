// The trust-region radius rule of Ceres 1.14's LevenbergMarquardtStrategy (StepAccepted / StepRejected) and TrustRegionMinimizer's count of
// consecutive invalid steps, as the host loops apply it: LmSolve (solver_lm.hpp) and lm_loop (lm_loop.hpp: the position and bundle solvers).  Plain arithmetic, no
// HIP: tests/cpp/trust_region_test.cpp builds it with the host compiler alone and replays an oracle trace through it bit for bit.
// The cube is std::pow(t, 3), the oracle's very call.  The device-side rules cube otherwise and differ in the last bit by design:
// k_lm_decide through lm_cube (correctly rounded), the per-track / per-edge / covariance kernels and host/evaluation.cpp by t * t * t.
#pragma once
#include <cmath>

struct TrustRegion {
  double radius = 0.0, decrease_factor = 2.0;
  int num_invalid = 0;   // consecutive invalid steps (the caller zeroes it at a valid one)
  // HandleInvalidStep: true on the fifth in a row (the solve fails), else the radius shrinks as for a rejected step
  bool invalid_step() {
    if (++num_invalid >= 5) return true;
    rejected();
    return false;
  }
  void rejected() { radius /= decrease_factor; decrease_factor *= 2.0; }
  void accepted(double rel_dec, double max_radius) {
    radius = radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rel_dec - 1.0, 3));
    radius = std::fmin(max_radius, radius);
    decrease_factor = 2.0;
  }
};
