// The host control loops of the position and bundle solvers (csrc/lm_loop.hpp), built by the host compiler alone.  lm_loop runs over an
// operations object that returns prescribed scalars and records its calls, pcg_loop over a prescribed sequence of r.M^-1 r, under both
// settings of its breakdown flag.  Prints PASSED.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_loop.hpp"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static const double NaN = std::nan(""), Inf = INFINITY;

// the fields lm_loop and pcg_loop read of gsfm_pos_options / gsfm_ba_options, and write of gsfm_pos_summary / gsfm_ba_summary
struct Options {
  int max_num_iterations = 50;
  double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32, min_relative_decrease = 1e-3;
  int max_cg_iterations = 100, cg_check_interval = 8;
  double cg_relative_tolerance = 1e-12;
  int cg_stall_iterations = 0, verbose = 0;
};
struct Summary {
  int termination = -1, num_iterations = -1, num_successful_steps = 0, num_unsuccessful_steps = 0, num_residual_sweeps = 0, num_linearizations = 0, nonfinite = 0;
  double initial_cost = 0, final_cost = 0, final_gradient_max_norm = 0, final_radius = 0, max_radius = 0;
};

// Scripted operations: the k-th call of an operation returns the k-th entry of its list.  `calls` spells the order: S start, s step,
// t trial cost, a accept.  fail_op / fail_at: that operation's call number fail_at (from 0) returns `status` instead.
struct Script {
  LmPoint at_start{100.0, 1.0, 100.0};
  std::vector<LmStep> steps;
  std::vector<double> trials;
  std::vector<LmPoint> accepts;
  char fail_op = 0;
  int fail_at = 0, status = 0;
  std::string calls;
  std::vector<double> radii;
  size_t n_step = 0, n_trial = 0, n_accept = 0;
  bool failing(char op, size_t k) { calls += op; return op == fail_op && (int)k == fail_at; }
  int start(LmPoint* at) { if (failing('S', 0)) return status; *at = at_start; return 0; }
  int step(double radius, LmStep* out) {
    radii.push_back(radius);
    if (failing('s', n_step)) return status;
    CHECK(n_step < steps.size());
    *out = steps[n_step++];
    return 0;
  }
  int trial_cost(double* cost) {
    if (failing('t', n_trial)) return status;
    CHECK(n_trial < trials.size());
    *cost = trials[n_trial++];
    return 0;
  }
  int accept(LmPoint* at) {
    if (failing('a', n_accept)) return status;
    CHECK(n_accept < accepts.size());
    at->gmax = accepts[n_accept].gmax; at->xnorm2 = accepts[n_accept].xnorm2;
    ++n_accept;
    return 0;
  }
};

// a valid step: |delta| = 1, model cost change -(-2) - 1 / 2 = 1.5
static const LmStep VALID{1.0, -2.0, 1.0, 3};
static const double MODEL = 1.5;

static int run(Script& sc, const Options& o, Summary* sum) { return lm_loop(sc, o, sum, "test"); }

static void test_lm_start() {
  {   // the gradient tolerance met at the start point
    Script sc; Options o; Summary s;
    sc.at_start = {5.0, 1e-11, 1.0};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_GRADIENT_TOLERANCE && s.num_iterations == 0 && s.num_residual_sweeps == 1 && s.num_linearizations == 1);
    CHECK(sc.calls == "S" && s.initial_cost == 5.0 && s.final_cost == 5.0 && s.final_gradient_max_norm == 1e-11 && s.nonfinite == 0);
    CHECK(s.final_radius == 1e4 && s.max_radius == 1e4);
  }
  for (double bad : {NaN, Inf}) {   // a start cost that is not finite
    Script sc; Options o; Summary s;
    sc.at_start = {bad, 1.0, 1.0};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_FAILURE && s.nonfinite == 1 && s.num_iterations == 0 && sc.calls == "S");
  }
}

static void test_lm_invalid_steps() {
  const double r = 1e4;
  {   // five in a row, of every kind: step2, delta.g or the quadratic term not finite; a model cost change of zero, and below zero
    Script sc; Options o; Summary s;
    sc.steps = {{NaN, -2.0, 1.0, 0}, {1.0, Inf, 1.0, 0}, {1.0, 0.0, 0.0, 0}, {1.0, 1.0, 1.0, 0}, {1.0, -2.0, NaN, 0}};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_FAILURE && s.num_iterations == 5 && s.num_unsuccessful_steps == 4 && s.num_successful_steps == 0);
    CHECK(sc.calls == "Ssssss" && sc.n_trial == 0 && s.num_residual_sweeps == 1 && s.nonfinite == 0);
    const double want[5] = {r, r / 2, r / 8, r / 64, r / 1024};
    CHECK(sc.radii.size() == 5);
    for (size_t k = 0; k < 5 && k < sc.radii.size(); ++k) CHECK(sc.radii[k] == want[k]);
    CHECK(s.final_radius == r / 1024 && s.final_cost == 100.0);
  }
  {   // a valid step between invalid ones restarts the count: 4 invalid, a rejected one, 4 invalid, an accepted one that meets the gradient tolerance
    Script sc; Options o; Summary s;
    const LmStep bad{1.0, 1.0, 1.0, 0};
    sc.steps = {bad, bad, bad, bad, VALID, bad, bad, bad, bad, VALID};
    sc.trials = {101.0, 99.0};
    sc.accepts = {{0.0, 1e-12, 100.0}};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_GRADIENT_TOLERANCE && s.num_iterations == 10 && s.num_unsuccessful_steps == 9 && s.num_successful_steps == 1);
    CHECK(sc.calls == std::string("S") + "ssss" + "st" + "ssss" + "sta");
    TrustRegion tr;
    tr.radius = r;
    for (size_t k = 0; k < sc.radii.size(); ++k) {
      CHECK(same_bits(sc.radii[k], tr.radius));
      if (k == 4) { tr.num_invalid = 0; tr.rejected(); }
      else if (k == 9) { tr.num_invalid = 0; tr.accepted((100.0 - 99.0) / MODEL, o.max_trust_region_radius); }
      else CHECK(!tr.invalid_step());
    }
    CHECK(same_bits(s.final_radius, tr.radius));
  }
}

static void test_lm_accept_reject_accept() {
  Script sc; Options o; Summary s;
  o.max_num_iterations = 3;
  o.initial_trust_region_radius = 3.0;
  sc.steps = {VALID, VALID, VALID};
  sc.trials = {99.0, 100.0, 98.2};     // from 100: accepted; from 99: rejected; from 99: accepted
  sc.accepts = {{0.0, 0.5, 81.0}, {0.0, 0.25, 64.0}};
  CHECK(run(sc, o, &s) == 0);
  CHECK(sc.calls == "Sstaststa" && sc.n_accept == 2);
  CHECK(s.termination == LM_TERM_NO_CONVERGENCE && s.num_iterations == 3 && s.num_successful_steps == 2 && s.num_unsuccessful_steps == 1);
  CHECK(s.num_residual_sweeps == 4 && s.num_linearizations == 3 && s.initial_cost == 100.0 && s.final_cost == 98.2 && s.final_gradient_max_norm == 0.25);
  TrustRegion tr;
  tr.radius = 3.0;
  double max_radius = tr.radius;
  const double x_cost[3] = {100.0, 99.0, 99.0};
  for (int k = 0; k < 3; ++k) {
    CHECK(same_bits(sc.radii[k], tr.radius));
    const double rel_dec = (x_cost[k] - sc.trials[k]) / MODEL;
    if (k == 1) tr.rejected(); else tr.accepted(rel_dec, o.max_trust_region_radius);
    max_radius = std::fmax(max_radius, tr.radius);
  }
  CHECK(same_bits(s.final_radius, tr.radius) && same_bits(s.max_radius, max_radius) && max_radius > 3.0);
}

static void test_lm_endings() {
  {   // parameter tolerance: the terminating step is counted and not applied
    Script sc; Options o; Summary s;
    sc.at_start = {100.0, 1.0, 1.0};
    sc.steps = {{1e-30, -2.0, 1.0, 0}};
    sc.trials = {99.0};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_PARAMETER_TOLERANCE && s.num_iterations == 1 && sc.calls == "Sst" && s.final_cost == 100.0);
    CHECK(s.num_successful_steps == 0 && s.num_unsuccessful_steps == 0 && s.num_residual_sweeps == 2 && s.num_linearizations == 1 && s.final_radius == 1e4);
  }
  {   // function tolerance: |cost change| <= 1e-6 x cost
    Script sc; Options o; Summary s;
    sc.steps = {VALID};
    sc.trials = {100.0 - 1e-5};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_FUNCTION_TOLERANCE && s.num_iterations == 1 && sc.calls == "Sst" && s.final_cost == 100.0 && s.num_successful_steps == 0);
  }
  {   // the gradient test between iterations: an accepted step whose gradient meets the tolerance ends the solve before another step; a
      // rejected step leaves the gradient of the start point, which did not meet it, and the solve goes on
    Script sc; Options o; Summary s;
    o.gradient_tolerance = 0.5;
    sc.steps = {VALID, VALID};
    sc.trials = {101.0, 99.0};
    sc.accepts = {{0.0, 0.5, 100.0}};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_GRADIENT_TOLERANCE && s.num_iterations == 2 && sc.calls == "Sststa" && s.final_cost == 99.0);
  }
  {   // a trial cost that is not finite counts as DBL_MAX: rejected
    Script sc; Options o; Summary s;
    o.max_num_iterations = 2;
    sc.steps = {VALID, VALID};
    sc.trials = {NaN, Inf};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_NO_CONVERGENCE && s.num_iterations == 2 && s.num_unsuccessful_steps == 2 && s.nonfinite == 1 && sc.calls == "Sstst");
    CHECK(s.final_cost == 100.0 && sc.radii[1] == 1e4 / 2 && s.final_radius == 1e4 / 8);
  }
  {   // the minimum radius
    Script sc; Options o; Summary s;
    o.min_trust_region_radius = 1e4 / 2;
    sc.steps = {VALID};
    sc.trials = {101.0};
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_FAILURE && s.num_iterations == 1 && sc.calls == "Sst" && s.final_radius == 1e4 / 2 && s.nonfinite == 0);
  }
  {   // max_num_iterations = 0: no step at all
    Script sc; Options o; Summary s;
    o.max_num_iterations = 0;
    o.verbose = 1;
    CHECK(run(sc, o, &s) == 0);
    CHECK(s.termination == LM_TERM_NO_CONVERGENCE && s.num_iterations == 0 && sc.calls == "S");
  }
}

static void test_lm_statuses() {
  // a status from any operation comes back unchanged, and nothing is called after it
  const struct { char op; int at; const char* calls; } cases[] = {{'S', 0, "S"}, {'s', 1, "Sstas"}, {'t', 1, "Sstast"}, {'a', 0, "Ssta"}};
  for (const auto& c : cases) {
    Script sc; Options o; Summary s;
    sc.fail_op = c.op; sc.fail_at = c.at; sc.status = 7;
    sc.steps = {VALID, VALID};
    sc.trials = {99.0, 98.0};
    sc.accepts = {{0.0, 1.0, 100.0}, {0.0, 1.0, 100.0}};
    CHECK(run(sc, o, &s) == 7);
    CHECK(sc.calls == c.calls);
    CHECK(s.termination == -1);   // (no summary of a solve that did not end)
  }
}

// ---- pcg_loop: rz[k] is r.M^-1 r after iteration k + 1 ----
struct Pcg {
  double slots[3] = {0, 0, 0};
  std::vector<double> rz;
  int it = 0, last_written = PCG_RZA, fail_read = -1;
  std::vector<int> read_at;   // the iteration count at every read after the first
  int n_reads = 0;
  int iters = -1; bool stalled = false; double rel = -1.0;
  int run(const Options& o, bool flag, double rz0) {
    slots[PCG_RZ0] = slots[PCG_RZA] = rz0;
    auto iterate = [&](int cur, int nxt) {
      CHECK(cur == last_written && nxt != cur && (nxt == PCG_RZA || nxt == PCG_RZB));
      CHECK((size_t)it < rz.size());
      slots[nxt] = rz[it++];
      last_written = nxt;
    };
    auto read = [&](int slot, double* v) {
      if (n_reads++ == fail_read) return 9;
      if (n_reads == 1) CHECK(slot == PCG_RZ0 && it == 0);
      else { CHECK(slot == last_written); read_at.push_back(it); }
      *v = slots[slot];
      return 0;
    };
    return pcg_loop(o, flag, iterate, read, &iters, &stalled, &rel);
  }
};

static void test_pcg() {
  for (bool flag : {false, true}) {
    {   // b = 0
      Pcg p; Options o;
      CHECK(p.run(o, flag, 0.0) == 0 && p.iters == 0 && !p.stalled && p.rel == 0.0 && p.it == 0);
    }
    for (double rz0 : {NaN, -3.0}) {   // a start value that is NaN or negative
      Pcg p; Options o;
      CHECK(p.run(o, flag, rz0) == 0 && p.iters == 0 && p.it == 0 && p.n_reads == 1);
      if (flag) CHECK(p.stalled && (std::isnan(rz0) ? std::isnan(p.rel) : p.rel == rz0));
      else CHECK(!p.stalled && p.rel == 0.0);   // recorded behaviour of pos_pcg: y = 0 passes as the solution
    }
    {   // looks only at multiples of cg_check_interval and at max_cg_iterations; no stall rule when cg_stall_iterations is 0
      Pcg p; Options o;
      o.max_cg_iterations = 20;
      p.rz.assign(20, 16.0);
      CHECK(p.run(o, flag, 16.0) == 0 && p.iters == 20 && p.stalled && p.rel == 1.0);
      CHECK(p.read_at == std::vector<int>({8, 16, 20}));
    }
    {   // convergence reports the iteration of the look that saw it
      Pcg p; Options o;
      o.cg_check_interval = 4;
      p.rz.assign(100, 1.0);
      for (int k = 9; k < 100; ++k) p.rz[k] = 16e-30;
      CHECK(p.run(o, flag, 16.0) == 0 && p.iters == 12 && !p.stalled && p.rel == std::sqrt(16e-30 / 16.0) && p.it == 12);
      CHECK(p.read_at == std::vector<int>({4, 8, 12}));
    }
    {   // the stall rule: cg_stall_iterations after the last quartering (iteration 3)
      Pcg p; Options o;
      o.cg_check_interval = 1; o.cg_stall_iterations = 5;
      p.rz.assign(100, 0.25);
      p.rz[0] = 4.0; p.rz[1] = 1.0;
      CHECK(p.run(o, flag, 16.0) == 0 && p.iters == 8 && p.stalled && p.rel == std::sqrt(0.25 / 16.0));
      Pcg q;
      o.cg_stall_iterations = 0; o.max_cg_iterations = 30;
      q.rz = p.rz;
      CHECK(q.run(o, flag, 16.0) == 0 && q.iters == 30 && q.stalled);
    }
    for (double bad : {NaN, Inf}) {   // r.M^-1 r not finite
      Pcg p; Options o;
      o.cg_check_interval = 1;
      p.rz = {4.0, 1.0, bad, 1.0};
      CHECK(p.run(o, flag, 16.0) == 0 && p.iters == 3 && p.stalled && (std::isnan(bad) ? std::isnan(p.rel) : p.rel == bad));
    }
    {   // r.M^-1 r negative in mid-run
      Pcg p; Options o;
      o.cg_check_interval = 1;
      p.rz = {4.0, -4.0, 1.0};
      CHECK(p.run(o, flag, 16.0) == 0 && p.iters == 2 && p.it == 2);
      if (flag) CHECK(p.stalled && p.rel == 0.5);   // sqrt(4 / 16): a breakdown
      // Recorded behaviour of pos_pcg, which never had the breakdown rule, not a goal: the negative value reads as a relative residual of
      // 0 and the solve ends as converged.
      else CHECK(!p.stalled && p.rel == 0.0);
    }
    for (int k : {0, 2}) {   // a status from a read comes back unchanged
      Pcg p; Options o;
      o.cg_check_interval = 1;
      p.rz.assign(10, 16.0);
      p.fail_read = k;
      CHECK(p.run(o, flag, 16.0) == 9 && p.it == k);
    }
  }
}

int main() {
  test_lm_start();
  test_lm_invalid_steps();
  test_lm_accept_reject_accept();
  test_lm_endings();
  test_lm_statuses();
  test_pcg();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("PASSED\n");
  return 0;
}
