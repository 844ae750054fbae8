// Host side of the bundle adjustment of camera positions and points (include/gsfm_ba.h): argument checks, the host structure
// (ba_structure.hpp), the Levenberg-Marquardt loop with Ceres 1.14's rules (the loop of pos_lm_solve, solver_pos.hpp; the radius rule is
// trust_region.hpp's) and the Schur-complement PCG.  The kernels are in ba_kernels.hpp; the vector kernels of the PCG and the reductions
// are the position problem's (pos_kernels.hpp), which work on any n x 3 array.
// Memory: one slab laid out by FlatLayout and owned, with the problem's private non-blocking stream, by a FlatCall member (flat_call.hpp).
// Every copy and memset is ordered on that stream.  The unknowns are one array of (n_cams + n_tracks) x 3, cameras first.
#pragma once
#include "host_common.hpp"
#include "flat_call.hpp"
#include "ba_structure.hpp"
#include "trust_region.hpp"
#include "triangulate.hpp"
#include "ba_kernels.hpp"
#include "../../include/gsfm_ba.h"

#include <memory>

struct gsfm_ba_problem {
  int device = 0;
  FlatCall mem;
  uint32_t n_cams = 0, n_tracks = 0;
  uint64_t n_obs = 0, n_used = 0;
  size_t n_nodes = 0;
  uint64_t n_active = 0;                     // active cameras + active points
  uint64_t cb[4] = {0, 0, 0, 0};             // the lane classes' slices of the launch order
  BaStructure st;                            // host copy of the active sets
  std::vector<uint8_t> h_active;             // n_nodes
  gsfm::DevLossNode leaf;
  // device arrays (ba_place)
  uint32_t *order = nullptr, *obs_cam = nullptr, *crow_ptr = nullptr, *cobs = nullptr, *ctrk = nullptr;
  uint64_t* track_ptr = nullptr;
  double2* obs_xy = nullptr;
  uint8_t *track_used = nullptr, *active = nullptr;
  double *cams = nullptr, *Ht = nullptr, *At = nullptr, *Hc = nullptr;
  // per node (3 or 6 doubles each)
  double *x = nullptr, *cand = nullptr, *g = nullptr, *Dg = nullptr, *S = nullptr, *D2 = nullptr, *b = nullptr, *y = nullptr, *delta = nullptr, *v = nullptr;
  // per camera
  double *rhs = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *Ap = nullptr, *Minv = nullptr;
  // per point
  double *Cinv = nullptr, *Cfix = nullptr, *Gt = nullptr, *zt = nullptr, *pt_scratch = nullptr;
  double *part = nullptr, *scal = nullptr;
  bool have_lin = false;
};

namespace {

using gsfm::BaDev;
using gsfm::BaSlots;

enum { BS_RZ0 = 0, BS_RZA = 1, BS_RZB = 2, BS_PAP = 3, BS_DV = 4, BS_VV = 5, BS_STEP2 = 6, BS_DG = 7, BS_DLD = 8, BS_COST = 9, BS_GMAX = 10,
       BS_XNORM2 = 11, BS_SUMD = 12 /* 3 */, BS_SUMX = 15 /* 3 */, BS_N = 18 };

BaDev ba_dev(const gsfm_ba_problem* P) {
  BaDev a{};
  a.n_cams = P->n_cams; a.n_tracks = P->n_tracks;
  a.track_ptr = P->track_ptr; a.obs_cam = P->obs_cam; a.obs_xy = P->obs_xy; a.cams = P->cams; a.track_used = P->track_used;
  a.crow_ptr = P->crow_ptr; a.cobs = P->cobs; a.ctrk = P->ctrk; a.active = P->active;
  a.Ht = P->Ht; a.At = P->At; a.Hc = P->Hc; a.leaf = P->leaf;
  return a;
}
// (at least one block: an empty launch is an error, and every kernel checks its bound)
inline dim3 ba_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + 255) / 256)); }
inline dim3 ba_row_grid(uint32_t n_cams) { return dim3(std::max(1u, (n_cams + 3) / 4)); }

// a point-side kernel over every track: one launch per lane class, the long tracks first (the order of triangulate.hpp)
template <typename K4, typename K16, typename K64, typename... Args>
void ba_tracks(const gsfm_ba_problem* P, K4 k4, K16 k16, K64 k64, Args... args) {
  const BaDev a = ba_dev(P);
  auto go = [&](int c, auto kernel, unsigned groups_per_block, unsigned block) {
    const BaSlots sl{P->cb[c + 1] - P->cb[c], P->order + P->cb[c]};
    if (sl.n_slots == 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((sl.n_slots + groups_per_block - 1) / groups_per_block)), dim3(block), 0, P->mem.s, a, sl, args...);
  };
  go(2, k64, 1, 64);
  go(1, k16, GSFM_TRI_BLOCK / 16, GSFM_TRI_BLOCK);
  go(0, k4, GSFM_TRI_BLOCK / 4, GSFM_TRI_BLOCK);
}
#define BA_TRACKS(P, K, ...) ba_tracks(P, K<4>, K<16>, K<64>, __VA_ARGS__)

int ba_read(gsfm_ba_problem* P, void* dst, const void* src_dev, size_t bytes, const char* what) {
  HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, P->mem.s));
  return sync_stream(P->mem.s, what);
}
void ba_reduce(gsfm_ba_problem* P, int slot, int is_max = 0) { hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, P->mem.s, P->part, P->scal + slot, is_max); }
// scal[slot] = a . b over n_rows x 3 entries (mask: per row), in a fixed order
void ba_dot(gsfm_ba_problem* P, const double* a, const double* b, const uint8_t* mask, size_t n_rows, int slot) {
  hipLaunchKernelGGL(k_pos_dot, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, a, b, mask, 3 * n_rows, P->part);
  ba_reduce(P, slot);
}
void ba_sum(gsfm_ba_problem* P, const double* a, size_t n, int slot) {
  hipLaunchKernelGGL(k_ba_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, a, n, P->part);
  ba_reduce(P, slot);
}

// cost of the point `at` into scal[BS_COST]
void ba_cost(gsfm_ba_problem* P, const double* at, double* r_out = nullptr, double* rho_out = nullptr) {
  BA_TRACKS(P, k_ba_cost_tracks, at, P->pt_scratch, r_out, rho_out);
  ba_sum(P, P->pt_scratch, P->n_tracks, BS_COST);
}
// linearisation at P->x: the point side evaluates every observation, the camera side copies the blocks into its order and sums its rows
void ba_linearize(gsfm_ba_problem* P) {
  BA_TRACKS(P, k_ba_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(k_ba_cam_lin, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, ba_dev(P), P->g, P->Dg);
}
void ba_norms(gsfm_ba_problem* P) {
  hipLaunchKernelGGL(k_pos_absmax, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, P->g, P->active, 3 * P->n_nodes, P->part);
  ba_reduce(P, BS_GMAX, 1);
  ba_dot(P, P->x, P->x, P->active, P->n_nodes, BS_XNORM2);
}

// D^2 at the radius, b = S g, the points' inverses (with what the right-hand side and the preconditioner need of them)
void ba_prep(gsfm_ba_problem* P, double radius, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_ba_prep_nodes, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, P->n_nodes, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal,
                     o.max_lm_diagonal, P->D2, P->b);
  hipLaunchKernelGGL(k_ba_prep_points, ba_grid(P->n_tracks), dim3(256), 0, P->mem.s, P->n_cams, P->n_tracks, P->active, P->Dg, P->S, P->D2, P->b, P->Cinv, P->Cfix, P->Gt,
                     P->zt);
}
// out = Sc v on the cameras, v = pvec and q = S pvec given: the point pass, then the camera pass
void ba_schur_product(gsfm_ba_problem* P, const double* qvec, const double* pvec, double* out) {
  BA_TRACKS(P, k_ba_point_pass, qvec, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)nullptr, P->zt, 1);
  hipLaunchKernelGGL(k_ba_cam_pass, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, ba_dev(P), qvec, (const double*)P->zt, pvec, (const double*)P->S,
                     (const double*)P->D2, (const double*)nullptr, out, 1);
}

// PCG on Sc y_c = rhs from y_c = 0 (k_ba_pcg_init set r, z, p, q); the loop of pos_pcg
int ba_pcg(gsfm_ba_problem* P, const gsfm_ba_options& o, int* iters, bool* stalled, double* rel) {
  *iters = 0; *stalled = false; *rel = 0.0;
  const uint32_t N = P->n_cams;
  ba_dot(P, P->r, P->z, nullptr, N, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  double rz0 = 0.0;
  if (int st = ba_read(P, &rz0, P->scal + BS_RZ0, 8, "pcg start")) return st;
  if (rz0 == 0.0) return 0;   // rhs = 0: y = 0 is the solution
  if (!(rz0 > 0.0) || !std::isfinite(rz0)) { *stalled = true; *rel = rz0; return 0; }   // NaN (the step is refused later) or a preconditioner that is not positive definite: y = 0 is no solution -- say so
  const int check = std::max(1, o.cg_check_interval);
  double best = rz0; int best_it = 0;
  int cur = BS_RZA, nxt = BS_RZB;
  int it = 0;
  while (it < o.max_cg_iterations) {
    ba_schur_product(P, P->q, P->p, P->Ap);
    ba_dot(P, P->p, P->Ap, nullptr, N, BS_PAP);
    hipLaunchKernelGGL(k_pos_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    ba_dot(P, P->r, P->z, nullptr, N, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
    std::swap(cur, nxt);
    ++it;
    if (it % check == 0 || it == o.max_cg_iterations) {
      double rz = 0.0;
      if (int st = ba_read(P, &rz, P->scal + cur, 8, "pcg")) return st;
      *rel = std::sqrt(std::fmax(rz, 0.0) / rz0);
      if (!std::isfinite(rz)) { *rel = rz; break; }
      if (rz < 0.0) { *rel = std::sqrt(-rz / rz0); break; }   // r.M^-1 r < 0: the system or its preconditioner is not positive definite as computed -- a breakdown, not a residual of zero
      if (*rel <= o.cg_relative_tolerance) { *iters = it; return 0; }
      if (rz <= 0.25 * best) { best = rz; best_it = it; }
      else if (o.cg_stall_iterations > 0 && it - best_it >= o.cg_stall_iterations) break;
    }
  }
  *iters = it;
  *stalled = true;
  return 0;
}

// One LM step's linear algebra at P->x, after its linearisation and with the Jacobi scale in place -- shared by the solve and by
// gsfm_ba_step_check.  Leaves y (cameras, then points), delta, the trial point P->cand and scal[BS_STEP2], [BS_DG], [BS_DLD] enqueued.
struct BaStep { int cg = 0; bool stalled = false; double cg_rel = 0.0; };
int ba_step(gsfm_ba_problem* P, double radius, const gsfm_ba_options& o, BaStep* out) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes;
  *out = BaStep();
  ba_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_ba_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)nullptr, (const double*)P->zt, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_ba_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Cfix, P->Minv);
  hipLaunchKernelGGL(k_ba_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = ba_pcg(P, o, &out->cg, &out->stalled, &out->cg_rel)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N), dim3(256), 0, P->mem.s, (size_t)N, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)P->b, P->y + 3 * (size_t)N, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  if (o.remove_gauge && P->n_active > 0) {
    for (int c = 0; c < 3; ++c) {
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)P->delta, P->active, NN, c, P->part);
      ba_reduce(P, BS_SUMD + c);
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)P->x, P->active, NN, c, P->part);
      ba_reduce(P, BS_SUMX + c);
    }
    hipLaunchKernelGGL(k_ba_center, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->scal, (int)BS_SUMD, (int)BS_SUMX, 1.0 / (double)P->n_active, P->x, P->delta, P->v);
  } else {
    HIPCHK(hipMemsetAsync(P->v, 0, 24 * NN, P->mem.s));
  }
  ba_dot(P, P->delta, P->v, nullptr, NN, BS_DV);
  ba_dot(P, P->v, P->v, nullptr, NN, BS_VV);
  hipLaunchKernelGGL(k_pos_project, ba_grid(NN), dim3(256), 0, P->mem.s, (uint32_t)NN, P->scal, BS_DV, BS_VV, P->v, P->delta, P->x, P->cand);
  ba_dot(P, P->delta, P->delta, nullptr, NN, BS_STEP2);
  ba_dot(P, P->delta, P->g, nullptr, NN, BS_DG);
  BA_TRACKS(P, k_ba_quad_tracks, (const double*)P->delta, P->pt_scratch);
  ba_sum(P, P->pt_scratch, T, BS_DLD);
  return 0;
}

int ba_lm_solve(gsfm_ba_problem* P, const gsfm_ba_options& o, gsfm_ba_summary* sum) {
  const size_t NN = P->n_nodes;
  TrustRegion tr;
  tr.radius = o.initial_trust_region_radius;
  int iteration = 0;
  double x_cost = 0.0, x_norm = 0.0, gmax = 0.0;
  double hs[BS_N];
  sum->max_radius = tr.radius;

  auto read_scal = [&](const char* what) { return ba_read(P, hs, P->scal, sizeof(hs), what); };
  auto finish = [&](int term) {
    sum->termination = term; sum->num_iterations = iteration; sum->final_cost = x_cost;
    sum->final_gradient_max_norm = gmax; sum->final_radius = tr.radius;
    if (!std::isfinite(x_cost)) sum->nonfinite = 1;
    return 0;
  };
  auto log = [&](double cost_change, double step_norm, double rel_dec, int cg) {
    if (o.verbose) fprintf(stderr, "[gsfm ba] it %3d cost %.12e dcost %.3e |g| %.3e |dx| %.3e rho %.3e radius %.3e cg %d\n",
                           iteration, x_cost, cost_change, gmax, step_norm, rel_dec, tr.radius, cg);
  };

  // iteration 0: cost, linearisation (with the Jacobi scale of the start point), gradient norm
  ba_cost(P, P->x);
  ba_linearize(P);
  hipLaunchKernelGGL(k_pos_scale, ba_grid(NN), dim3(256), 0, P->mem.s, (uint32_t)NN, P->Dg, P->S, o.jacobi_scaling);
  ba_norms(P);
  if (int st = read_scal("start point")) return st;
  x_cost = hs[BS_COST]; gmax = hs[BS_GMAX]; x_norm = std::sqrt(hs[BS_XNORM2]);
  sum->num_residual_sweeps++; sum->num_linearizations++;
  sum->initial_cost = x_cost;
  log(0, 0, 0, 0);
  if (!std::isfinite(x_cost)) return finish(GSFM_TERM_FAILURE);
  if (gmax <= o.gradient_tolerance) return finish(GSFM_TERM_GRADIENT_TOLERANCE);
  bool last_successful = false;
  while (true) {
    if (iteration >= o.max_num_iterations) return finish(GSFM_TERM_NO_CONVERGENCE);
    if (last_successful && gmax <= o.gradient_tolerance) return finish(GSFM_TERM_GRADIENT_TOLERANCE);
    if (tr.radius <= o.min_trust_region_radius) return finish(GSFM_TERM_FAILURE);
    ++iteration;
    last_successful = false;
    BaStep step;
    if (int st = ba_step(P, tr.radius, o, &step)) return st;
    const int cg = step.cg;
    sum->num_cg_iterations += cg;
    if (step.stalled) sum->num_pcg_stalled_steps++;
    if (int st = read_scal("step")) return st;
    const double step2 = hs[BS_STEP2];
    bool valid = std::isfinite(step2) && std::isfinite(hs[BS_DG]) && std::isfinite(hs[BS_DLD]);
    // model cost change -(J delta)^T (r + J delta / 2) = -delta.g - delta^T L delta / 2
    const double model_cost_change = -hs[BS_DG] - 0.5 * hs[BS_DLD];
    if (valid && !(model_cost_change > 0.0)) valid = false;
    if (!valid) {   // HandleInvalidStep
      if (tr.invalid_step()) return finish(GSFM_TERM_FAILURE);
      sum->num_unsuccessful_steps++;
      log(0, 0, 0, cg);
      continue;
    }
    tr.num_invalid = 0;
    double cand_cost = 0.0;
    ba_cost(P, P->cand);
    if (int st = ba_read(P, &cand_cost, P->scal + BS_COST, 8, "trial cost")) return st;
    sum->num_residual_sweeps++;
    if (!std::isfinite(cand_cost)) { cand_cost = std::numeric_limits<double>::max(); sum->nonfinite = 1; }
    const double step_norm = std::sqrt(step2);
    const double cost_change = x_cost - cand_cost;
    const double rel_dec = cost_change / model_cost_change;
    if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { log(cost_change, step_norm, rel_dec, cg); return finish(GSFM_TERM_PARAMETER_TOLERANCE); }
    if (std::fabs(cost_change) <= o.function_tolerance * x_cost) { log(cost_change, step_norm, rel_dec, cg); return finish(GSFM_TERM_FUNCTION_TOLERANCE); }
    if (rel_dec > o.min_relative_decrease) {   // HandleSuccessfulStep
      HIPCHK(hipMemcpyAsync(P->x, P->cand, 24 * NN, hipMemcpyDeviceToDevice, P->mem.s));
      x_cost = cand_cost;
      ba_linearize(P);
      ba_norms(P);
      if (int st = read_scal("linearisation")) return st;
      gmax = hs[BS_GMAX]; x_norm = std::sqrt(hs[BS_XNORM2]);
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

gsfm_ba_options ba_options(const gsfm_ba_options* opt) {
  gsfm_ba_options o;
  if (opt) return *opt;
  gsfm_ba_options_default(&o);
  return o;
}

// x = (cam_pos, points), enqueued
int ba_upload_point(gsfm_ba_problem* P, const double* cam_pos, const double* points) {
  if (P->n_cams) HIPCHK(hipMemcpyAsync(P->x, cam_pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->mem.s));
  if (P->n_tracks) HIPCHK(hipMemcpyAsync(P->x + 3 * (size_t)P->n_cams, points, 24 * (size_t)P->n_tracks, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}
// what a solve does before its first step: cost and linearisation at the point given, the Jacobi scale of that point
int ba_setup_linearize(gsfm_ba_problem* P, const double* cam_pos, const double* points, const gsfm_ba_options& o, double* cost) {
  if (int st = ba_upload_point(P, cam_pos, points)) return st;
  ba_cost(P, P->x);
  ba_linearize(P);
  hipLaunchKernelGGL(k_pos_scale, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, (uint32_t)P->n_nodes, P->Dg, P->S, o.jacobi_scaling);
  if (int st = ba_read(P, cost, P->scal + BS_COST, 8, "linearisation")) return st;
  P->have_lin = true;
  return 0;
}
bool ba_needs_points(const gsfm_ba_problem* P, const double* cam_pos, const double* points) {
  return (P->n_cams > 0 && !cam_pos) || (P->n_tracks > 0 && !points);
}

// ---- problem creation ----
int ba_check_create(uint32_t n_cams, const double* rot_aa, const double* intrinsics, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                    const double* obs_xy) {
  if (n_cams > 0 && (!rot_aa || !intrinsics)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!track_ptr) return fail(GSFM_ERR_INVALID_ARG, "NULL argument (track_ptr holds n_tracks + 1 entries)");
  if (track_ptr[0] != 0) return fail(GSFM_ERR_INVALID_ARG, "track_ptr[0] must be 0");
  for (uint64_t t = 0; t < n_tracks; ++t)
    if (track_ptr[t + 1] < track_ptr[t]) return fail(GSFM_ERR_INVALID_ARG, "track_ptr decreases at track " + std::to_string(t));
  const uint64_t O = track_ptr[n_tracks];
  if (O >= (1ull << 31) || (uint64_t)n_cams + n_tracks >= (1ull << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 observations or nodes)");
  if (O > 0 && (!obs_cam || !obs_xy)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t k = 0; k < O; ++k)
    if (obs_cam[k] >= n_cams) return fail(GSFM_ERR_INVALID_ARG, "observation " + std::to_string(k) + " has an out-of-range camera index");
  if (const char* why = no_device_reason("gsfm_ba_problem_create")) return fail(GSFM_ERR_NO_DEVICE, why);
  return 0;
}

// The arrays of the slab in order: laid out (slab == NULL), then pointed into the committed slab.  *zeroed: the bytes one memset clears.
FlatLayout ba_place(gsfm_ba_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  FlatLayout L;
  auto take = [&](auto*& ptr, size_t count) {
    using E = std::remove_reference_t<decltype(*ptr)>;
    const Slot<E> slot = L.take<E>(count);
    if (slab) ptr = (E*)(slab + slot.off);
  };
  take(P->scal, BS_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta, &P->v}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 3 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Cfix, GSFM_BA_FIX_DOUBLES * T);   // (no point is flagged before the first k_ba_prep_points)
  *zeroed = L.total;
  take(P->Minv, 9 * N); take(P->Cinv, 9 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS);
  take(P->cams, GSFM_TRI_CAM_DOUBLES * N); take(P->Ht, 6 * O); take(P->At, 3 * O); take(P->Hc, 6 * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN);
  return L;
}

gsfm_status ba_create_impl(uint32_t n_cams, const double* rot_aa, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks,
                           const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (int st = ba_check_create(n_cams, rot_aa, intrinsics, n_tracks, track_ptr, obs_cam, obs_xy)) return (gsfm_status)st;
  const size_t N = n_cams, T = n_tracks, O = track_ptr[n_tracks];
  hvec<uint32_t> order(T);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1);
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<gsfm_ba_problem, void (*)(gsfm_ba_problem*)> P(new gsfm_ba_problem, gsfm_ba_problem_destroy);
  (void)hipGetDevice(&P->device);
  P->n_cams = n_cams; P->n_tracks = (uint32_t)n_tracks; P->n_obs = O; P->n_nodes = N + T;
  P->st = ba_build_structure(n_cams, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated);
  P->n_used = P->st.n_used;
  P->n_active = (uint64_t)P->st.n_active_cams + P->st.n_active_points;
  P->h_active.resize(N + T);
  std::copy(P->st.cam_active.begin(), P->st.cam_active.end(), P->h_active.begin());
  std::copy(P->st.point_active.begin(), P->st.point_active.end(), P->h_active.begin() + N);
  tri_bucket(T, track_ptr, order.data(), P->cb);
  std::memset(&P->leaf, 0, sizeof(P->leaf));
  P->leaf.kind = GSFM_LOSS_TRIVIAL;

  size_t zeroed = 0;
  if (int st = P->mem.commit(ba_place(P.get(), nullptr, &zeroed), "the bundle adjustment problem", 0)) return (gsfm_status)st;
  ba_place(P.get(), P->mem.slab, &zeroed);
  const hipStream_t s = P->mem.s;
  HIPCHK_S(hipMemsetAsync(P->mem.slab, 0, zeroed, s));
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
  HIPCHK_S(up(P->track_ptr, track_ptr, 8 * (T + 1))); HIPCHK_S(up(P->order, order.data(), 4 * T));
  HIPCHK_S(up(P->obs_cam, obs_cam, 4 * O)); HIPCHK_S(up(P->obs_xy, obs_xy, 16 * O));
  HIPCHK_S(up(P->crow_ptr, P->st.row_ptr.data(), 4 * (N + 1))); HIPCHK_S(up(P->cobs, P->st.obs.data(), 4 * P->n_used)); HIPCHK_S(up(P->ctrk, P->st.trk.data(), 4 * P->n_used));
  HIPCHK_S(up(P->track_used, P->st.track_used.data(), T)); HIPCHK_S(up(P->active, P->h_active.data(), N + T));
  // the camera records from rot_aa and f u v (positions are unknowns: the record's position field stays zero); staged in cand / g / D2, x still zero
  if (N > 0) {
    HIPCHK_S(up(P->cand, rot_aa, 24 * N)); HIPCHK_S(up(P->g, intrinsics, 24 * N));
    HIPCHK_S(up(P->D2, est.data(), N));
    hipLaunchKernelGGL(k_tri_cameras, ba_grid(N), dim3(256), 0, s, n_cams, (const double*)P->cand, (const double*)P->x, (const double*)P->g, (const uint8_t*)P->D2, P->cams);
    HIPCHK_S(hipMemsetAsync(P->mem.slab, 0, zeroed, s));
  }
  if (int st = sync_stream(s, "bundle adjustment problem create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

gsfm_status ba_solve_impl(gsfm_ba_problem* P, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = ba_options(opt);
  gsfm_ba_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->num_observations_used = P->n_used; summary->num_active_cameras = P->st.n_active_cams; summary->num_active_points = P->st.n_active_points;
  summary->termination = GSFM_TERM_GRADIENT_TOLERANCE;
  if (P->n_used == 0) return GSFM_OK;   // nothing to adjust: nothing changes
  const double t0 = now_ms();
  const size_t N = P->n_cams, T = P->n_tracks;
  if (int st = ba_upload_point(P, cam_pos, points)) return (gsfm_status)st;
  if (int st = ba_lm_solve(P, o, summary)) return (gsfm_status)st;
  hvec<double> xh(3 * (N + T));
  if (int st = ba_read(P, xh.data(), P->x, 24 * (N + T), "download the estimates")) return (gsfm_status)st;
  // only the active nodes are parameters: every other row of the caller's arrays keeps its bytes
  for (size_t k = 0; k < N; ++k) if (P->h_active[k]) std::copy(&xh[3 * k], &xh[3 * k] + 3, cam_pos + 3 * k);
  for (size_t t = 0; t < T; ++t) if (P->h_active[N + t]) std::copy(&xh[3 * (N + t)], &xh[3 * (N + t)] + 3, points + 3 * t);
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status ba_linearize_impl(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                              double* diag_cam, double* diag_point) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = N + T;
  gsfm_ba_options o;
  gsfm_ba_options_default(&o);
  double c = 0.0;
  if (int st = ba_setup_linearize(P, cam_pos, points, o, &c)) return (gsfm_status)st;
  hvec<double> g3(3 * NN), d6(6 * NN);
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g, 24 * NN, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg, 48 * NN, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearize outputs")) return (gsfm_status)st;
  if (grad_cam) std::copy(g3.begin(), g3.begin() + 3 * N, grad_cam);
  if (grad_point) std::copy(g3.begin() + 3 * N, g3.end(), grad_point);
  auto full = [&](size_t node, double* dst) {
    const double* m = &d6[6 * node];
    const double f9[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
    std::copy(f9, f9 + 9, dst);
  };
  if (diag_cam) for (size_t k = 0; k < N; ++k) full(k, diag_cam + 9 * k);
  if (diag_point) for (size_t t = 0; t < T; ++t) full(N + t, diag_point + 9 * t);
  if (cost) *cost = c;
  return GSFM_OK;
}

gsfm_status ba_residuals_impl(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t O = P->n_obs;
  if (O == 0) return GSFM_OK;
  FlatLayout L;
  const Slot<double> r = L.take<double>(2 * O), rho = L.take<double>(O);
  DevBuf<char> scratch;
  if (scratch.alloc(L.total) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  if (int st = ba_upload_point(P, cam_pos, points)) return (gsfm_status)st;
  ba_cost(P, P->x, (double*)(scratch.p + r.off), (double*)(scratch.p + rho.off));
  if (r_out) HIPCHK_S(hipMemcpyAsync(r_out, scratch.p + r.off, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (rho_out) HIPCHK_S(hipMemcpyAsync(rho_out, scratch.p + rho.off, 8 * O, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "residuals");
}

}  // namespace

extern "C" {

int gsfm_ba_abi_version(void) { return GSFM_BA_ABI_VERSION; }

void gsfm_ba_options_default(gsfm_ba_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 100; o->jacobi_scaling = 1;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e12; o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
  o->max_cg_iterations = 2000; o->cg_check_interval = 8; o->cg_relative_tolerance = 1e-12; o->cg_stall_iterations = 200;
  o->remove_gauge = 1; o->verbose = 0;
}

gsfm_status gsfm_ba_time_kernels(gsfm_ba_problem* P, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us) {
  if (!P || !out_us || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  DeviceGuard g(P->device);
  gsfm_ba_options o;
  gsfm_ba_options_default(&o);
  double cost = 0.0;
  if (int st = ba_setup_linearize(P, cam_pos, points, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = ba_step(P, radius, o, &step)) return (gsfm_status)st;
  hipEvent_t e0, e1;
  HIPCHK_S(hipEventCreate(&e0)); HIPCHK_S(hipEventCreate(&e1));
  const uint32_t N = P->n_cams;
  int st = 0, k = 0;
  auto timed = [&](auto launch) {
    if (st) return;
    launch();   // warm
    (void)hipEventRecord(e0, P->mem.s);
    for (int r = 0; r < reps; ++r) launch();
    (void)hipEventRecord(e1, P->mem.s);
    st = sync_stream(P->mem.s, "time_kernels");
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    out_us[k++] = 1e3 * ms / reps;
  };
  timed([&] { BA_TRACKS(P, k_ba_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_lin, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), P->g, P->Dg); });
  timed([&] { BA_TRACKS(P, k_ba_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)nullptr, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->q, (const double*)P->zt, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Cfix, P->Minv); });
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return (gsfm_status)st;
}

void gsfm_ba_problem_destroy(gsfm_ba_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

gsfm_status gsfm_ba_problem_create(uint32_t n_cams, const double* rot_aa, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks,
                                   const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                   gsfm_ba_problem** out) {
  return guarded("bundle adjustment problem creation", ba_create_impl, n_cams, rot_aa, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 point_estimated, out);
}

gsfm_status gsfm_ba_set_loss(gsfm_ba_problem* P, const gsfm_loss_node* prog, int32_t n) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || n > 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the bundle adjustment takes a loss of one leaf (composite programs are not supported)");
  // Every refusal below returns before P is read or written (the ABI tests hand in a handle that is no problem at all): keep the checks
  // ahead of the first use of P.
  gsfm::DevLossNode leaf;
  std::memset(&leaf, 0, sizeof(leaf));
  leaf.kind = GSFM_LOSS_TRIVIAL;
  if (n == 1) {
    const int k = prog[0].kind;
    if (!(k == GSFM_LOSS_TRIVIAL || k == GSFM_LOSS_HUBER || k == GSFM_LOSS_SOFT_L1 || k == GSFM_LOSS_TUKEY || k == GSFM_LOSS_GEMAN_MCCLURE))
      return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the bundle adjustment takes the losses Trivial, Huber, SoftLOne, Tukey and GemanMcClure (MAGSAC and the other leaves are not supported)");
    for (int j = 0; j < 3; ++j) {
      if (!std::isfinite(prog[0].p[j])) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "loss parameter is not finite");
      leaf.p[j] = prog[0].p[j];
    }
    if (k != GSFM_LOSS_TRIVIAL && !(prog[0].p[0] > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the loss width must be positive");
    leaf.kind = k;
  }
  P->leaf = leaf;   // (passed to the kernels by value)
  P->have_lin = false;
  return GSFM_OK;
}

gsfm_status gsfm_ba_solve(gsfm_ba_problem* P, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  return guarded("the bundle adjustment", ba_solve_impl, P, cam_pos, points, opt, summary);
}

gsfm_status gsfm_ba_residuals(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  return guarded("bundle adjustment residuals", ba_residuals_impl, P, cam_pos, points, r_out, rho_out);
}

gsfm_status gsfm_ba_linearize(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                              double* diag_cam, double* diag_point) {
  return guarded("bundle adjustment linearisation", ba_linearize_impl, P, cam_pos, points, cost, grad_cam, grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_ba_schur_matvec(gsfm_ba_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_ba_linearize or gsfm_ba_step_check first");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = ba_options(opt);
  const size_t N = P->n_cams;
  if (N == 0) return GSFM_OK;
  hipLaunchKernelGGL(k_pos_scale, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, (uint32_t)P->n_nodes, P->Dg, P->S, o.jacobi_scaling);
  ba_prep(P, radius, o);
  HIPCHK_S(hipMemcpyAsync(P->p, v, 24 * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->S, P->p, 1.0, P->q);
  ba_schur_product(P, P->q, P->p, P->Ap);
  HIPCHK_S(hipMemcpyAsync(y, P->Ap, 24 * N, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "schur_matvec");
}

gsfm_status gsfm_ba_step_check(gsfm_ba_problem* P, const double* cam_pos, const double* points, double radius, const gsfm_ba_options* opt, double* rhs_out,
                               double* yc_out, double* yp_out, double* delta_cam_out, double* delta_point_out, double* scal_out, int32_t* info_out) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = ba_options(opt);
  const size_t N = P->n_cams, T = P->n_tracks;
  double cost = 0.0;
  if (int st = ba_setup_linearize(P, cam_pos, points, o, &cost)) return (gsfm_status)st;
  BaStep step;
  if (int st = ba_step(P, radius, o, &step)) return (gsfm_status)st;
  double hs[BS_N];
  auto down = [&](double* dst, const double* src, size_t rows) { return (dst && rows) ? hipMemcpyAsync(dst, src, 24 * rows, hipMemcpyDeviceToHost, P->mem.s) : hipSuccess; };
  HIPCHK_S(hipMemcpyAsync(hs, P->scal, sizeof(hs), hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(down(rhs_out, P->rhs, N)); HIPCHK_S(down(yc_out, P->y, N)); HIPCHK_S(down(yp_out, P->y + 3 * N, T));
  HIPCHK_S(down(delta_cam_out, P->delta, N)); HIPCHK_S(down(delta_point_out, P->delta + 3 * N, T));
  if (int st = sync_stream(P->mem.s, "step check")) return (gsfm_status)st;
  if (scal_out) {
    scal_out[0] = -hs[BS_DG] - 0.5 * hs[BS_DLD];   // the solve's model cost change
    scal_out[1] = hs[BS_DG]; scal_out[2] = hs[BS_DLD]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.cg; info_out[1] = step.stalled ? 1 : 0; }
  return GSFM_OK;
}

}  // extern "C"
