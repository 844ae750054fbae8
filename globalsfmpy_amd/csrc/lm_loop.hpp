// The host control loops of the Euclidean solvers -- positions (solver_pos.hpp), positions and points (solver_ba.hpp), orientations, positions
// and points (solver_full_ba.hpp) -- once: lm_loop, Ceres 1.14's TrustRegionMinimizer + LevenbergMarquardtStrategy restated from
// oracle/ref_solver.cpp::lm_solve for Euclidean parameters (the radius rule is trust_region.hpp's), and pcg_loop, the driver of their
// preconditioned conjugate gradients.  Plain arithmetic over a few callables, no HIP: tests/cpp/lm_loop_test.cpp builds this header with the
// host compiler alone and drives every branch with scripted scalars.  The rotation solver's LmSolve (solver_lm.hpp: forcing schedule,
// components, graph replay) is another loop.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>

#include "trust_region.hpp"

// gsfm_rot.h's GSFM_TERM_* by value (solver_pos.hpp asserts it)
enum { LM_TERM_FUNCTION_TOLERANCE = 0, LM_TERM_GRADIENT_TOLERANCE = 1, LM_TERM_PARAMETER_TOLERANCE = 2, LM_TERM_NO_CONVERGENCE = 3, LM_TERM_FAILURE = 4 };

struct LmPoint { double cost = 0.0, gmax = 0.0, xnorm2 = 0.0; };   // cost, gradient max norm and |x|^2 over the free parameters
struct LmStep { double step2 = 0.0, dg = 0.0, quad = 0.0; int cg = 0; };   // |delta|^2, delta.g, delta^T (J^T J) delta; PCG iterations (the log line)

// What a solver gives the loop; every call returns a status, and a non-zero one ends the loop at once with that status.
//   int start(LmPoint*)               cost, linearisation, Jacobi scale and norms at x, enqueued and read back (cost, gmax, xnorm2)
//   int step(double radius, LmStep*)  one step's linear algebra at the radius, with the solver's own count of PCG iterations, stalls and
//                                     dense solves, and the three scalars of the decision read back; leaves the candidate on the device
//   int trial_cost(double*)           the candidate's cost, read back
//   int accept(LmPoint*)              x = candidate, linearisation and norms there, read back (gmax, xnorm2; cost is not touched)
// O: gsfm_pos_options or gsfm_ba_options; Sum: gsfm_pos_summary or gsfm_ba_summary.  tag: the solver's name in the verbose line.
template <typename Ops, typename O, typename Sum>
int lm_loop(Ops& ops, const O& o, Sum* sum, const char* tag) {
  TrustRegion tr;
  tr.radius = o.initial_trust_region_radius;
  int iteration = 0;
  double x_cost = 0.0, x_norm = 0.0, gmax = 0.0;
  sum->max_radius = tr.radius;

  auto finish = [&](int term) {
    sum->termination = term; sum->num_iterations = iteration; sum->final_cost = x_cost;
    sum->final_gradient_max_norm = gmax; sum->final_radius = tr.radius;
    if (!std::isfinite(x_cost)) sum->nonfinite = 1;
    return 0;
  };
  auto log = [&](double cost_change, double step_norm, double rel_dec, int cg) {
    if (o.verbose) fprintf(stderr, "[gsfm %s] it %3d cost %.12e dcost %.3e |g| %.3e |dx| %.3e rho %.3e radius %.3e cg %d\n",
                           tag, iteration, x_cost, cost_change, gmax, step_norm, rel_dec, tr.radius, cg);
  };

  // iteration 0: cost, linearisation (with the Jacobi scale of the start point), gradient norm
  LmPoint at;
  if (int st = ops.start(&at)) return st;
  x_cost = at.cost; gmax = at.gmax; x_norm = std::sqrt(at.xnorm2);
  sum->num_residual_sweeps++; sum->num_linearizations++;
  sum->initial_cost = x_cost;
  log(0, 0, 0, 0);
  if (!std::isfinite(x_cost)) return finish(LM_TERM_FAILURE);
  if (gmax <= o.gradient_tolerance) return finish(LM_TERM_GRADIENT_TOLERANCE);
  bool last_successful = false;
  while (true) {
    if (iteration >= o.max_num_iterations) return finish(LM_TERM_NO_CONVERGENCE);
    if (last_successful && gmax <= o.gradient_tolerance) return finish(LM_TERM_GRADIENT_TOLERANCE);
    if (tr.radius <= o.min_trust_region_radius) return finish(LM_TERM_FAILURE);
    ++iteration;
    last_successful = false;
    LmStep step;
    if (int st = ops.step(tr.radius, &step)) return st;
    const int cg = step.cg;
    const double step2 = step.step2;
    bool valid = std::isfinite(step2) && std::isfinite(step.dg) && std::isfinite(step.quad);
    // model cost change -(J delta)^T (r + J delta / 2) = -delta.g - delta^T (J^T J) delta / 2
    const double model_cost_change = -step.dg - 0.5 * step.quad;
    if (valid && !(model_cost_change > 0.0)) valid = false;
    if (!valid) {   // HandleInvalidStep
      if (tr.invalid_step()) return finish(LM_TERM_FAILURE);
      sum->num_unsuccessful_steps++;
      log(0, 0, 0, cg);
      continue;
    }
    tr.num_invalid = 0;
    double cand_cost = 0.0;
    if (int st = ops.trial_cost(&cand_cost)) return st;
    sum->num_residual_sweeps++;
    if (!std::isfinite(cand_cost)) { cand_cost = std::numeric_limits<double>::max(); sum->nonfinite = 1; }
    const double step_norm = std::sqrt(step2);
    const double cost_change = x_cost - cand_cost;
    const double rel_dec = cost_change / model_cost_change;
    if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { log(cost_change, step_norm, rel_dec, cg); return finish(LM_TERM_PARAMETER_TOLERANCE); }
    if (std::fabs(cost_change) <= o.function_tolerance * x_cost) { log(cost_change, step_norm, rel_dec, cg); return finish(LM_TERM_FUNCTION_TOLERANCE); }
    if (rel_dec > o.min_relative_decrease) {   // HandleSuccessfulStep
      x_cost = cand_cost;
      if (int st = ops.accept(&at)) return st;
      gmax = at.gmax; x_norm = std::sqrt(at.xnorm2);
      sum->num_linearizations++;
      tr.accepted(rel_dec, o.max_trust_region_radius);
      sum->num_successful_steps++;
      last_successful = true;
    } else {   // HandleUnsuccessfulStep
      tr.rejected();
      sum->num_unsuccessful_steps++;
    }
    sum->max_radius = std::fmax(sum->max_radius, tr.radius);
    log(cost_change, step_norm, rel_dec, cg);
  }
}

// The slots of a solver's device scalars that the PCG recurrence uses: r.M^-1 r of the start, and of the last two iterations in turn
enum { PCG_RZ0 = 0, PCG_RZA = 1, PCG_RZB = 2 };

// PCG from y = 0, after the caller has enqueued r.M^-1 r into the slots PCG_RZ0 and PCG_RZA.
//   void iterate(int cur, int nxt)    enqueue one iteration: it reads r.M^-1 r in slot cur and writes the new one to slot nxt
//   int read(int slot, double* v)     slot's value, waited for
// *iters: the iterations run; *stalled: ended above the tolerance; *rel: the last relative residual read back, sqrt(r.M^-1 r / b.M^-1 b) of
// the recursion (0 when b = 0).  O: cg_check_interval (a look every so many iterations), max_cg_iterations, cg_relative_tolerance,
// cg_stall_iterations (without a quartering of r.M^-1 r for so many iterations the solve gives up; 0: never).
// breakdown_is_stall: what a r.M^-1 r that is not positive means.  true (both bundle adjustments): the system or its preconditioner is not
// positive definite as computed, so a start value that is negative or NaN, and a negative value later, end the solve as stalled, with
// *rel = the start value, or sqrt(-r.M^-1 r / b.M^-1 b).  false (the position solver, whose pos_pcg never had the breakdown rule): such a
// start returns y = 0 as solved and a negative value later reads as a relative residual of 0, converged.
template <typename O, typename Iterate, typename Read>
int pcg_loop(const O& o, bool breakdown_is_stall, Iterate iterate, Read read, int* iters, bool* stalled, double* rel) {
  *iters = 0; *stalled = false; *rel = 0.0;
  double rz0 = 0.0;
  if (int st = read(PCG_RZ0, &rz0)) return st;
  if (rz0 == 0.0) return 0;   // b = 0: y = 0 is the solution
  if (!(rz0 > 0.0) || !std::isfinite(rz0)) {   // (a NaN right-hand side: the step is refused later)
    if (breakdown_is_stall) { *stalled = true; *rel = rz0; }   // y = 0 is no solution -- say so
    return 0;
  }
  const int check = o.cg_check_interval > 1 ? o.cg_check_interval : 1;
  double best = rz0; int best_it = 0;
  int cur = PCG_RZA, nxt = PCG_RZB;
  int it = 0;
  while (it < o.max_cg_iterations) {
    iterate(cur, nxt);
    const int t = cur; cur = nxt; nxt = t;
    ++it;
    if (it % check == 0 || it == o.max_cg_iterations) {
      double rz = 0.0;
      if (int st = read(cur, &rz)) return st;
      *rel = std::sqrt(std::fmax(rz, 0.0) / rz0);
      if (!std::isfinite(rz)) { *rel = rz; break; }
      if (breakdown_is_stall && rz < 0.0) { *rel = std::sqrt(-rz / rz0); break; }   // a breakdown, not a residual of zero
      if (*rel <= o.cg_relative_tolerance) { *iters = it; return 0; }
      if (rz <= 0.25 * best) { best = rz; best_it = it; }   // the relative residual sqrt(rz / rz0) halved
      else if (o.cg_stall_iterations > 0 && it - best_it >= o.cg_stall_iterations) break;
    }
  }
  *iters = it;
  *stalled = true;
  return 0;
}
