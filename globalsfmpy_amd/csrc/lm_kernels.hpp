// Device-side Levenberg-Marquardt control for exact steps: the CT_* slots of the control block, LmOpts, k_lm_decide, k_lm_after.
// Launched by the device-controlled loop in solver_lm.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_math.hpp"

namespace gsfm {

// ------------------------------------------------------------------------------------------
// Device-side Levenberg-Marquardt control for EXACT steps (latency regime: Madrid-sized graphs, one Cholesky step per iteration).  The
// decisions of TrustRegionMinimizer the host loop takes between two synchronisations -- step validity, the two tolerance tests, acceptance,
// the radius law -- are taken by one lane from the scalars the step and cost kernels left on the device; the kernels of the accept path (state
// copy, linearisation) are predicated on its verdict and the damping is rebuilt from the radius it wrote, so a whole LM iteration is
// enqueued without a host decision and read back ONCE (solver_lm.hpp).  Same formulas, same operation order as the host loop: the two
// controls produce bit-identical trajectories (tests/test_gpu_round4.py).
// ------------------------------------------------------------------------------------------
enum { CT_RADIUS = 0, CT_DF = 1, CT_XCOST = 2, CT_XNORM = 3, CT_GMAX = 4, CT_ACCEPT = 5, CT_TERM = 6 /* -1: go on */, CT_NINVALID = 7, CT_VALID = 8,
       CT_CAND = 9, CT_CC = 10, CT_MCC = 11, CT_STEPN = 12, CT_DENSE_FAIL = 13, CT_NONFINITE = 14, CT_SKIPPED = 15 /* this iteration was enqueued ahead of a verdict that ended the run: nothing was decided */, CT_N = 16 };
struct LmOpts { double function_tolerance, gradient_tolerance, parameter_tolerance, min_relative_decrease, max_radius, min_radius; };
// (2 rel_dec - 1)^3 of the radius law as Ceres rounds it: std::pow(t, 3) is the correctly rounded cube (glibc: < 0.52 ulp), t * t * t is two roundings.
// t^2 = h + l and h t = p + e exactly (FMA residues), the cube is p + (e + l t): one rounding of a value good to 2^-100, i.e. the correctly rounded
// result but for ties nobody will meet -- the device's radius trace equals the oracle's bit for bit (tests/test_gpu_round5.py).
__device__ __forceinline__ double lm_cube(double t) {
#pragma clang fp contract(off)   // (under the device default, -ffp-contract=fast, `p + fma(l, t, e)` becomes fma(h, t, fma(l, t, e)), which counts the residue e twice;
                                 // HIP's __dmul_rn / __dadd_rn are plain operators and do not stop it)
  const double h = t * t, l = fma(t, t, -h);
  const double p = h * t, e = fma(h, t, -p);
  return p + fma(l, t, e);
}
// `it_dev`: the number of the LM iteration the next k_lm_after stamps its record with -- on the device, so that no kernel of an iteration takes a
// per-iteration argument and the whole iteration replays as one hipGraph (solver_lm.hpp)
__global__ void k_set_double(double* p, double v) { *p = v; }   // one device word from a host value, in stream order (no staging buffer to keep alive)
__global__ void k_lm_set(double* ctl, double radius, double df, double x_cost, double x_norm, double gmax, double n_invalid, double* it_dev, double iteration) {
  *it_dev = iteration;
  ctl[CT_RADIUS] = radius; ctl[CT_DF] = df; ctl[CT_XCOST] = x_cost; ctl[CT_XNORM] = x_norm; ctl[CT_GMAX] = gmax; ctl[CT_NINVALID] = n_invalid;
  ctl[CT_ACCEPT] = 0.0; ctl[CT_TERM] = -1.0; ctl[CT_DENSE_FAIL] = 0.0; ctl[CT_NONFINITE] = 0.0; ctl[CT_SKIPPED] = 0.0;
}
// scal: SC_STEP.. = eta.g, eta.r, eta^T Lam eta, |delta|^2, |x_trial|^2 ; trial cost ; dense status.  (indices passed in: the enum lives on the host side)
// The control block is authoritative between host interventions (k_lm_set): iteration k + 1 may be enqueued before the host has read
// iteration k's verdict, so a verdict that ends the run of exact steps -- a termination, a factor that broke down -- must stop every later
// decision: such an iteration is marked SKIPPED, accepts nothing and leaves the block alone.
__device__ __forceinline__ void lm_decide_body(const LmOpts& o, const double* scal, int sc_step, int sc_trial, int sc_info, double* ctl) {
  ctl[CT_ACCEPT] = 0.0;
  if (ctl[CT_TERM] >= 0.0 || ctl[CT_DENSE_FAIL] != 0.0) { ctl[CT_SKIPPED] = 1.0; return; }
  ctl[CT_SKIPPED] = 0.0; ctl[CT_VALID] = 0.0; ctl[CT_NONFINITE] = 0.0;
  int info;
  __builtin_memcpy(&info, scal + sc_info, sizeof(int));
  if (info != 0) { ctl[CT_DENSE_FAIL] = 1.0; return; }   // the factor broke down: the step is meaningless, the host solves it again by PCG
  const double eta_g = scal[sc_step], eta_r = scal[sc_step + 1], eta_L = scal[sc_step + 2];
  const double mcc = -0.5 * eta_g + 0.5 * eta_r + 0.5 * eta_L;
  ctl[CT_MCC] = mcc;
  double radius = ctl[CT_RADIUS], df = ctl[CT_DF];
  if (!(isfinite(mcc) && mcc > 0.0)) {   // HandleInvalidStep
    const double ni = ctl[CT_NINVALID] + 1.0;
    ctl[CT_NINVALID] = ni;
    if (ni >= 5.0) { ctl[CT_TERM] = 4.0; return; }
    ctl[CT_RADIUS] = radius / df; ctl[CT_DF] = df * 2.0;
    return;
  }
  ctl[CT_VALID] = 1.0; ctl[CT_NINVALID] = 0.0;
  double cand = scal[sc_trial];
  if (!isfinite(cand)) { cand = 1.7976931348623157e308; ctl[CT_NONFINITE] = 1.0; }
  const double x_cost = ctl[CT_XCOST], x_norm = ctl[CT_XNORM];
  const double step_norm = sqrt(scal[sc_step + 3]), cost_change = x_cost - cand, rel_dec = cost_change / mcc;
  ctl[CT_CAND] = cand; ctl[CT_CC] = cost_change; ctl[CT_STEPN] = step_norm;
  if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { ctl[CT_TERM] = 2.0; return; }
  if (fabs(cost_change) <= o.function_tolerance * x_cost) { ctl[CT_TERM] = 0.0; return; }
  if (rel_dec > o.min_relative_decrease) {   // HandleSuccessfulStep
    ctl[CT_ACCEPT] = 1.0;
    ctl[CT_XNORM] = sqrt(scal[sc_step + 4]); ctl[CT_XCOST] = cand;
    radius = radius / fmax(1.0 / 3.0, 1.0 - lm_cube(2.0 * rel_dec - 1.0));
    ctl[CT_RADIUS] = fmin(o.max_radius, radius); ctl[CT_DF] = 2.0;
  } else { ctl[CT_RADIUS] = radius / df; ctl[CT_DF] = df * 2.0; }
}
// One workgroup closes the step: the five sums of k_cam_step's partials and the trial cost's (the reductions k_sum_partials_multi /
// k_sum_partials would have launched: same routine, same order, same bits, written to the same scalars), the decision (one lane), and -- if the
// step is accepted -- x <- x_trial, q <- q_trial (copies, not pointer swaps: captured graphs hold the addresses).  Three launches fewer per
// exact LM iteration than sum, sum, decide, accept (~4.5 us each on a chain of ~60 dependent launches).
__global__ void __launch_bounds__(GSFM_BLOCK) k_lm_decide(LmOpts o, double* scal, int sc_step, int sc_trial, int sc_info, double* ctl,
                                                          const double* __restrict__ step_part, int nb_cam, const double* __restrict__ cost_part, int nb_cost,
                                                          uint32_t n, int param_dim, double* x, const double* __restrict__ x_trial, double2* q, const double2* __restrict__ q_trial) {
  __shared__ double lds[8];
  for (int c = 0; c < 5; ++c) {
    const double t = sum_partials_bcast(step_part + (size_t)c * nb_cam, nb_cam, lds);
    if (threadIdx.x == 0) scal[sc_step + c] = t;
  }
  {
    const double t = sum_partials_bcast(cost_part, nb_cost, lds);
    if (threadIdx.x == 0) scal[sc_trial] = t;
  }
  if (threadIdx.x == 0) {
    lm_decide_body(o, scal, sc_step, sc_trial, sc_info, ctl);
    lds[5] = ctl[CT_ACCEPT];
  }
  __syncthreads();
  if (lds[5] == 0.0) return;
  for (uint32_t k = threadIdx.x; k < n; k += GSFM_BLOCK) {
    for (int c = 0; c < param_dim; ++c) x[(size_t)param_dim * k + c] = x_trial[(size_t)param_dim * k + c];
    q[2 * (size_t)k] = q_trial[2 * (size_t)k]; q[2 * (size_t)k + 1] = q_trial[2 * (size_t)k + 1];
  }
}
// after the (predicated) linearisation and the damping rebuild: the gradient test of an accepted step, the radius floor
// ... and the iteration's record for the host: the control block as this iteration left it, in its slot of a ring (the host reads it from a
// side stream while the next iteration is already running).  `gterm`: the gradient / radius verdicts are kept apart from CT_TERM in the record
// (the host loop takes them at the top of the NEXT iteration, after recording this one) but halt later decisions just the same.
// `rec` is host memory mapped into the device (the host polls the record's last word instead of synchronising a stream: a cross-stream event
// costs tens of microseconds per iteration, more than the gap it was meant to close); `stamp` = the LM iteration, written last, system scope.
// (round 4: the max-norm reduction of k_cam_prep's partials -- k_max_partials, same routine -- is done here, one launch fewer)
__global__ void __launch_bounds__(GSFM_BLOCK) k_lm_after(LmOpts o, double* scal, int sc_gmax, double* ctl, double* rec_ring, int rec_stride, double* it_dev, const double* __restrict__ gmax_part, int nb_cam) {
  __shared__ double lds[8];
  {
    double v = 0.0;
    for (int k = threadIdx.x; k < nb_cam; k += GSFM_BLOCK) v = fmax(v, gmax_part[k]);
    const double t = block_max_bcast(v, lds);
    if (threadIdx.x != 0) return;
    scal[sc_gmax] = t;
  }
  if (ctl[CT_SKIPPED] != 0.0) return;
  const double stamp = *it_dev;                                  // this iteration's number; the next one's is one more
  double* const rec = rec_ring + (size_t)rec_stride * ((int)stamp & 3);
  *it_dev = stamp + 1.0;
  double term_next = -1.0;
  if (ctl[CT_TERM] < 0.0 && ctl[CT_DENSE_FAIL] == 0.0) {
    if (ctl[CT_ACCEPT] != 0.0) {
      ctl[CT_GMAX] = scal[sc_gmax];
      if (ctl[CT_GMAX] <= o.gradient_tolerance) term_next = 1.0;
    }
    if (term_next < 0.0 && ctl[CT_RADIUS] <= o.min_radius) term_next = 4.0;
  }
  for (int k = 0; k < CT_N; ++k) rec[k] = ctl[k];
  __threadfence_system();
  __hip_atomic_store(rec + CT_N, stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (term_next >= 0.0) ctl[CT_TERM] = term_next;   // (after the copy: the record shows the iteration's own verdict)
}

}  // namespace gsfm
