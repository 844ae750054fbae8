// Host side of the full bundle adjustment (include/gsfm_ba6.h): orientations, positions and points.  The loop is solver_ba.hpp's -- argument
// checks, ba_structure.hpp's host structure, Ceres 1.14's LM rules with trust_region.hpp's radius rule, the Schur-complement PCG with the
// recurrence and the vector kernels of pos_kernels.hpp -- over the kernels of ba6_kernels.hpp, plus the seven-direction gauge projection
// whose 7 x 7 Gram system is solved here.
// Memory: one slab laid out by FlatLayout and owned, with the problem's private non-blocking stream, by a FlatCall member (flat_call.hpp).
// Every copy and memset is ordered on that stream.  The unknowns are one array of (2 n_cams + n_tracks) x 3: angle-axis vectors, centres,
// points.
#pragma once
#include "solver_ba.hpp"
#include "ba6_kernels.hpp"
#include "../../include/gsfm_ba6.h"

struct gsfm_ba6_problem {
  int device = 0;
  FlatCall mem;
  uint32_t n_cams = 0, n_tracks = 0;
  uint64_t n_obs = 0, n_used = 0;
  size_t n_nodes = 0;                        // 2 n_cams + n_tracks
  uint64_t n_active_pp = 0;                  // active centres + active points (the nodes the centroid runs over)
  uint64_t cb[4] = {0, 0, 0, 0};
  BaStructure st;
  std::vector<uint8_t> h_active;             // n_nodes
  gsfm::DevLossNode leaf;
  uint32_t *order = nullptr, *obs_cam = nullptr, *crow_ptr = nullptr, *cobs = nullptr, *ctrk = nullptr;
  uint64_t* track_ptr = nullptr;
  double2* obs_xy = nullptr;
  uint8_t *track_used = nullptr, *active = nullptr, *cam_est = nullptr;
  double *cams = nullptr, *intrinsics = nullptr, *Jt = nullptr, *Rt = nullptr, *Jc = nullptr, *Bx = nullptr;
  // per node (3 or 6 doubles each)
  double *x = nullptr, *cand = nullptr, *g = nullptr, *Dg = nullptr, *S = nullptr, *D2 = nullptr, *b = nullptr, *y = nullptr, *delta = nullptr;
  // per camera node (2 n_cams x 3)
  double *rhs = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *Ap = nullptr, *Minv = nullptr;
  // per point
  double *Cinv = nullptr, *Gt = nullptr, *zt = nullptr, *pt_scratch = nullptr;
  double *part = nullptr, *gpart = nullptr, *scal = nullptr;
  bool have_lin = false;
};

namespace {

using gsfm::Ba6Dev;

enum { B6_RZ0 = 0, B6_RZA = 1, B6_RZB = 2, B6_PAP = 3, B6_STEP2 = 4, B6_DG = 5, B6_JD2 = 6, B6_COST = 7, B6_GMAX = 8, B6_XNORM2 = 9,
       B6_SUMX = 10 /* 3 */, B6_COEF = 13 /* 7 */, B6_GRAM = 20 /* 35 */, B6_N = 55 };

Ba6Dev b6_dev(const gsfm_ba6_problem* P) {
  Ba6Dev a{};
  a.b.n_cams = P->n_cams; a.b.n_tracks = P->n_tracks;
  a.b.track_ptr = P->track_ptr; a.b.obs_cam = P->obs_cam; a.b.obs_xy = P->obs_xy; a.b.cams = P->cams; a.b.track_used = P->track_used;
  a.b.crow_ptr = P->crow_ptr; a.b.cobs = P->cobs; a.b.ctrk = P->ctrk; a.b.active = P->active; a.b.leaf = P->leaf;
  a.Jt = P->Jt; a.Rt = P->Rt; a.Jc = P->Jc;
  return a;
}

template <typename K4, typename K16, typename K64, typename... Args>
void b6_tracks(const gsfm_ba6_problem* P, K4 k4, K16 k16, K64 k64, Args... args) {
  const Ba6Dev a = b6_dev(P);
  auto go = [&](int c, auto kernel, unsigned groups_per_block, unsigned block) {
    const BaSlots sl{P->cb[c + 1] - P->cb[c], P->order + P->cb[c]};
    if (sl.n_slots == 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((sl.n_slots + groups_per_block - 1) / groups_per_block)), dim3(block), 0, P->mem.s, a, sl, args...);
  };
  go(2, k64, 1, 64);
  go(1, k16, GSFM_TRI_BLOCK / 16, GSFM_TRI_BLOCK);
  go(0, k4, GSFM_TRI_BLOCK / 4, GSFM_TRI_BLOCK);
}
#define B6_TRACKS(P, K, ...) b6_tracks(P, K<4>, K<16>, K<64>, __VA_ARGS__)

int b6_read(gsfm_ba6_problem* P, void* dst, const void* src_dev, size_t bytes, const char* what) {
  HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, P->mem.s));
  return sync_stream(P->mem.s, what);
}
void b6_reduce(gsfm_ba6_problem* P, int slot, int is_max = 0) { hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, P->mem.s, P->part, P->scal + slot, is_max); }
void b6_dot(gsfm_ba6_problem* P, const double* a, const double* b, const uint8_t* mask, size_t n_rows, int slot) {
  hipLaunchKernelGGL(k_pos_dot, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, a, b, mask, 3 * n_rows, P->part);
  b6_reduce(P, slot);
}
void b6_sum(gsfm_ba6_problem* P, const double* a, size_t n, int slot) {
  hipLaunchKernelGGL(k_ba_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, a, n, P->part);
  b6_reduce(P, slot);
}
// the camera records (R, J_l) of the point `at`
void b6_cameras(gsfm_ba6_problem* P, const double* at) {
  if (P->n_cams) hipLaunchKernelGGL(k_ba6_cameras, ba_grid(P->n_cams), dim3(256), 0, P->mem.s, P->n_cams, at, (const double*)P->intrinsics, (const uint8_t*)P->cam_est, P->cams);
}
// cost of the point `at` into scal[B6_COST]
void b6_cost(gsfm_ba6_problem* P, const double* at, double* r_out = nullptr, double* rho_out = nullptr) {
  b6_cameras(P, at);
  B6_TRACKS(P, k_ba6_cost_tracks, at, P->pt_scratch, r_out, rho_out);
  b6_sum(P, P->pt_scratch, P->n_tracks, B6_COST);
}
void b6_linearize(gsfm_ba6_problem* P) {
  b6_cameras(P, P->x);
  B6_TRACKS(P, k_ba6_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(k_ba6_cam_lin, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, b6_dev(P), P->g, P->Dg, P->Bx);
}
void b6_norms(gsfm_ba6_problem* P) {
  hipLaunchKernelGGL(k_pos_absmax, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, P->g, P->active, 3 * P->n_nodes, P->part);
  b6_reduce(P, B6_GMAX, 1);
  b6_dot(P, P->x, P->x, P->active, P->n_nodes, B6_XNORM2);
}
void b6_jacobi_scale(gsfm_ba6_problem* P, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_pos_scale, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, (uint32_t)P->n_nodes, P->Dg, P->S, o.jacobi_scaling);
}
void b6_prep(gsfm_ba6_problem* P, double radius, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_ba_prep_nodes, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, P->n_nodes, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal,
                     o.max_lm_diagonal, P->D2, P->b);
  // (the points are the nodes from 2 n_cams on; their inverses are refined: ba6_kernels.hpp)
  hipLaunchKernelGGL(k_ba6_prep_points, ba_grid(P->n_tracks), dim3(256), 0, P->mem.s, 2 * P->n_cams, P->n_tracks, P->active, P->Dg, P->S, P->D2, P->b, P->Cinv,
                     P->Gt, P->zt);
}
void b6_schur_product(gsfm_ba6_problem* P, const double* qvec, const double* pvec, double* out) {
  B6_TRACKS(P, k_ba6_point_pass, qvec, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1);
  hipLaunchKernelGGL(k_ba6_cam_pass, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, b6_dev(P), qvec, (const double*)P->zt, 1.0, pvec, (const double*)P->S,
                     (const double*)P->D2, (const double*)nullptr, out, 1);
}

// PCG on Sc y_c = rhs from y_c = 0 (k_ba6_pcg_init set r, z, p, q); the loop of ba_pcg over the cameras' 2 N nodes
int b6_pcg(gsfm_ba6_problem* P, const gsfm_ba_options& o, int* iters, bool* stalled, double* rel) {
  *iters = 0; *stalled = false; *rel = 0.0;
  const uint32_t N = P->n_cams, N2 = 2 * N;
  b6_dot(P, P->r, P->z, nullptr, N2, B6_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + B6_RZA, P->scal + B6_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  double rz0 = 0.0;
  if (int st = b6_read(P, &rz0, P->scal + B6_RZ0, 8, "pcg start")) return st;
  if (rz0 == 0.0) return 0;                                   // rhs = 0: y = 0 is the solution
  if (!(rz0 > 0.0) || !std::isfinite(rz0)) { *stalled = true; *rel = rz0; return 0; }   // NaN, or a preconditioner that is not positive definite: y = 0 is no solution -- say so
  const int check = std::max(1, o.cg_check_interval);
  double best = rz0; int best_it = 0;
  int cur = B6_RZA, nxt = B6_RZB;
  int it = 0;
  while (it < o.max_cg_iterations) {
    b6_schur_product(P, P->q, P->p, P->Ap);
    b6_dot(P, P->p, P->Ap, nullptr, N2, B6_PAP);
    hipLaunchKernelGGL(k_ba6_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, B6_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    b6_dot(P, P->r, P->z, nullptr, N2, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N2), dim3(256), 0, P->mem.s, N2, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
    std::swap(cur, nxt);
    ++it;
    if (it % check == 0 || it == o.max_cg_iterations) {
      double rz = 0.0;
      if (int st = b6_read(P, &rz, P->scal + cur, 8, "pcg")) return st;
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

// (V^T V) c = V^T delta by Cholesky without pivoting; a direction whose pivot is not above 1e-12 of its own squared norm keeps c = 0
void b6_gauge_solve(const double* dots, double* c) {
  const int n = GSFM_BA6_GAUGE;
  double A[GSFM_BA6_GAUGE][GSFM_BA6_GAUGE], L[GSFM_BA6_GAUGE][GSFM_BA6_GAUGE] = {}, w[GSFM_BA6_GAUGE];
  bool keep[GSFM_BA6_GAUGE];
  int q = 0;
  for (int i = 0; i < n; ++i) for (int j = i; j < n; ++j) { A[i][j] = dots[q]; A[j][i] = dots[q]; ++q; }
  for (int j = 0; j < n; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) if (keep[k]) d -= L[j][k] * L[j][k];
    keep[j] = std::isfinite(d) && d > 1e-12 * A[j][j];
    if (!keep[j]) continue;
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < n; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) if (keep[k]) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  for (int i = 0; i < n; ++i) {   // L w = V^T delta
    w[i] = 0.0;
    if (!keep[i]) continue;
    double s = dots[28 + i];
    for (int k = 0; k < i; ++k) if (keep[k]) s -= L[i][k] * w[k];
    w[i] = s / L[i][i];
  }
  for (int i = n - 1; i >= 0; --i) {   // L^T c = w
    c[i] = 0.0;
    if (!keep[i]) continue;
    double s = w[i];
    for (int k = i + 1; k < n; ++k) if (keep[k]) s -= L[k][i] * c[k];
    c[i] = s / L[i][i];
  }
}

// One LM step's linear algebra at P->x, after its linearisation and with the Jacobi scale in place -- shared by the solve and by
// gsfm_ba6_step_check.  Leaves y, delta, the trial point P->cand and scal[B6_STEP2], [B6_DG], [B6_JD2] enqueued.  jd_out: device, may be NULL.
int b6_step(gsfm_ba6_problem* P, double radius, const gsfm_ba_options& o, BaStep* out, double* jd_out = nullptr) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes;
  *out = BaStep();
  b6_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_ba6_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)nullptr, (const double*)P->zt, -1.0, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_ba6_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv);
  hipLaunchKernelGGL(k_ba6_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = b6_pcg(P, o, &out->cg, &out->stalled, &out->cg_rel)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(2 * (size_t)N), dim3(256), 0, P->mem.s, 2 * (size_t)N, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) B6_TRACKS(P, k_ba6_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->b, -1.0, P->y + 6 * (size_t)N, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  const bool project = o.remove_gauge && P->n_active_pp > 0;
  const double inv_count = P->n_active_pp > 0 ? 1.0 / (double)P->n_active_pp : 0.0;
  if (project) {
    for (int c = 0; c < 3; ++c) {
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)(P->x + 3 * (size_t)N), P->active + N, (size_t)N + T, c, P->part);
      b6_reduce(P, B6_SUMX + c);
    }
    hipLaunchKernelGGL(k_ba6_gauge_dots, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->delta,
                       (const double*)P->scal, (int)B6_SUMX, inv_count, P->gpart);
    hipLaunchKernelGGL(k_ba6_gauge_reduce, dim3(GSFM_BA6_GDOTS), dim3(256), 0, P->mem.s, (const double*)P->gpart, P->scal + B6_GRAM);
    double dots[GSFM_BA6_GDOTS], coef[GSFM_BA6_GAUGE];
    if (int st = b6_read(P, dots, P->scal + B6_GRAM, sizeof(dots), "gauge dots")) return st;
    b6_gauge_solve(dots, coef);
    HIPCHK(hipMemcpyAsync(P->scal + B6_COEF, coef, sizeof(coef), hipMemcpyHostToDevice, P->mem.s));
    if (int st = sync_stream(P->mem.s, "gauge coefficients")) return st;   // (coef is a local)
  }
  hipLaunchKernelGGL(k_ba6_gauge_apply, ba_grid(NN), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->scal, (int)B6_SUMX, inv_count,
                     (int)B6_COEF, project ? 1 : 0, P->delta, P->cand);
  b6_dot(P, P->delta, P->delta, nullptr, NN, B6_STEP2);
  b6_dot(P, P->delta, P->g, nullptr, NN, B6_DG);
  B6_TRACKS(P, k_ba6_quad_tracks, (const double*)P->delta, P->pt_scratch, jd_out);
  b6_sum(P, P->pt_scratch, T, B6_JD2);
  return 0;
}

int b6_lm_solve(gsfm_ba6_problem* P, const gsfm_ba_options& o, gsfm_ba_summary* sum) {
  const size_t NN = P->n_nodes;
  TrustRegion tr;
  tr.radius = o.initial_trust_region_radius;
  int iteration = 0;
  double x_cost = 0.0, x_norm = 0.0, gmax = 0.0;
  double hs[B6_N];
  sum->max_radius = tr.radius;

  auto read_scal = [&](const char* what) { return b6_read(P, hs, P->scal, sizeof(hs), what); };
  auto finish = [&](int term) {
    sum->termination = term; sum->num_iterations = iteration; sum->final_cost = x_cost;
    sum->final_gradient_max_norm = gmax; sum->final_radius = tr.radius;
    if (!std::isfinite(x_cost)) sum->nonfinite = 1;
    return 0;
  };
  auto log = [&](double cost_change, double step_norm, double rel_dec, int cg) {
    if (o.verbose) fprintf(stderr, "[gsfm ba6] it %3d cost %.12e dcost %.3e |g| %.3e |dx| %.3e rho %.3e radius %.3e cg %d\n",
                           iteration, x_cost, cost_change, gmax, step_norm, rel_dec, tr.radius, cg);
  };

  // iteration 0: cost, linearisation (with the Jacobi scale of the start point), gradient norm
  b6_cost(P, P->x);
  b6_linearize(P);
  b6_jacobi_scale(P, o);
  b6_norms(P);
  if (int st = read_scal("start point")) return st;
  x_cost = hs[B6_COST]; gmax = hs[B6_GMAX]; x_norm = std::sqrt(hs[B6_XNORM2]);
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
    if (int st = b6_step(P, tr.radius, o, &step)) return st;
    const int cg = step.cg;
    sum->num_cg_iterations += cg;
    if (step.stalled) sum->num_pcg_stalled_steps++;
    if (int st = read_scal("step")) return st;
    const double step2 = hs[B6_STEP2];
    bool valid = std::isfinite(step2) && std::isfinite(hs[B6_DG]) && std::isfinite(hs[B6_JD2]);
    // model cost change -(J delta)^T (r + J delta / 2) = -delta.g - |J delta|^2 / 2
    const double model_cost_change = -hs[B6_DG] - 0.5 * hs[B6_JD2];
    if (valid && !(model_cost_change > 0.0)) valid = false;
    if (!valid) {   // HandleInvalidStep
      if (tr.invalid_step()) return finish(GSFM_TERM_FAILURE);
      sum->num_unsuccessful_steps++;
      log(0, 0, 0, cg);
      continue;
    }
    tr.num_invalid = 0;
    double cand_cost = 0.0;
    b6_cost(P, P->cand);
    if (int st = b6_read(P, &cand_cost, P->scal + B6_COST, 8, "trial cost")) return st;
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
      b6_linearize(P);
      b6_norms(P);
      if (int st = read_scal("linearisation")) return st;
      gmax = hs[B6_GMAX]; x_norm = std::sqrt(hs[B6_XNORM2]);
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

gsfm_ba_options b6_options(const gsfm_ba_options* opt) {
  gsfm_ba_options o;
  if (opt) return *opt;
  gsfm_ba6_options_default(&o);
  return o;
}

// x = (rot_aa, cam_pos, points), enqueued
int b6_upload_point(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points) {
  const size_t N = P->n_cams;
  if (N) {
    HIPCHK(hipMemcpyAsync(P->x, rot_aa, 24 * N, hipMemcpyHostToDevice, P->mem.s));
    HIPCHK(hipMemcpyAsync(P->x + 3 * N, cam_pos, 24 * N, hipMemcpyHostToDevice, P->mem.s));
  }
  if (P->n_tracks) HIPCHK(hipMemcpyAsync(P->x + 6 * N, points, 24 * (size_t)P->n_tracks, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}
int b6_setup_linearize(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, const gsfm_ba_options& o, double* cost) {
  if (int st = b6_upload_point(P, rot_aa, cam_pos, points)) return st;
  b6_cost(P, P->x);
  b6_linearize(P);
  b6_jacobi_scale(P, o);
  if (int st = b6_read(P, cost, P->scal + B6_COST, 8, "linearisation")) return st;
  P->have_lin = true;
  return 0;
}
bool b6_needs_points(const gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points) {
  return (P->n_cams > 0 && (!rot_aa || !cam_pos)) || (P->n_tracks > 0 && !points);
}

FlatLayout b6_place(gsfm_ba6_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  FlatLayout L;
  auto take = [&](auto*& ptr, size_t count) {
    using E = std::remove_reference_t<decltype(*ptr)>;
    const Slot<E> slot = L.take<E>(count);
    if (slab) ptr = (E*)(slab + slot.off);
  };
  take(P->scal, B6_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 6 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Bx, 9 * N);
  *zeroed = L.total;
  take(P->Minv, 36 * N); take(P->Cinv, 18 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS); take(P->gpart, (size_t)GSFM_BA6_GDOTS * GSFM_POS_PARTS);
  take(P->cams, GSFM_BA6_CAM_DOUBLES * N); take(P->intrinsics, 3 * N); take(P->Jt, 12 * O); take(P->Rt, 2 * O); take(P->Jc, 12 * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN); take(P->cam_est, N);
  return L;
}

// the argument checks of gsfm_ba6_problem_create, on the host before any device call (the rules of gsfm_ba_problem_create; a camera is two nodes)
int b6_check_create(uint32_t n_cams, const double* intrinsics, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy) {
  if (n_cams > 0 && !intrinsics) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!track_ptr) return fail(GSFM_ERR_INVALID_ARG, "NULL argument (track_ptr holds n_tracks + 1 entries)");
  if (track_ptr[0] != 0) return fail(GSFM_ERR_INVALID_ARG, "track_ptr[0] must be 0");
  for (uint64_t t = 0; t < n_tracks; ++t)
    if (track_ptr[t + 1] < track_ptr[t]) return fail(GSFM_ERR_INVALID_ARG, "track_ptr decreases at track " + std::to_string(t));
  const uint64_t O = track_ptr[n_tracks];
  if (O >= (1ull << 31) || (uint64_t)2 * n_cams + n_tracks >= (1ull << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 observations or nodes)");
  if (O > 0 && (!obs_cam || !obs_xy)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t k = 0; k < O; ++k)
    if (obs_cam[k] >= n_cams) return fail(GSFM_ERR_INVALID_ARG, "observation " + std::to_string(k) + " has an out-of-range camera index");
  if (const char* why = no_device_reason("gsfm_ba6_problem_create")) return fail(GSFM_ERR_NO_DEVICE, why);
  return 0;
}

gsfm_status b6_create_impl(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                           const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba6_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (int st = b6_check_create(n_cams, intrinsics, n_tracks, track_ptr, obs_cam, obs_xy)) return (gsfm_status)st;
  const size_t N = n_cams, T = n_tracks, O = track_ptr[n_tracks];
  hvec<uint32_t> order(T);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1);
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<gsfm_ba6_problem, void (*)(gsfm_ba6_problem*)> P(new gsfm_ba6_problem, gsfm_ba6_problem_destroy);
  (void)hipGetDevice(&P->device);
  P->n_cams = n_cams; P->n_tracks = (uint32_t)n_tracks; P->n_obs = O; P->n_nodes = 2 * N + T;
  P->st = ba_build_structure(n_cams, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated);
  P->n_used = P->st.n_used;
  P->n_active_pp = (uint64_t)P->st.n_active_cams + P->st.n_active_points;
  P->h_active.resize(2 * N + T);
  std::copy(P->st.cam_active.begin(), P->st.cam_active.end(), P->h_active.begin());
  std::copy(P->st.cam_active.begin(), P->st.cam_active.end(), P->h_active.begin() + N);
  std::copy(P->st.point_active.begin(), P->st.point_active.end(), P->h_active.begin() + 2 * N);
  tri_bucket(T, track_ptr, order.data(), P->cb);
  std::memset(&P->leaf, 0, sizeof(P->leaf));
  P->leaf.kind = GSFM_LOSS_TRIVIAL;

  size_t zeroed = 0;
  if (int st = P->mem.commit(b6_place(P.get(), nullptr, &zeroed), "the full bundle adjustment problem", 0)) return (gsfm_status)st;
  b6_place(P.get(), P->mem.slab, &zeroed);
  const hipStream_t s = P->mem.s;
  HIPCHK_S(hipMemsetAsync(P->mem.slab, 0, zeroed, s));
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
  HIPCHK_S(up(P->track_ptr, track_ptr, 8 * (T + 1))); HIPCHK_S(up(P->order, order.data(), 4 * T));
  HIPCHK_S(up(P->obs_cam, obs_cam, 4 * O)); HIPCHK_S(up(P->obs_xy, obs_xy, 16 * O));
  HIPCHK_S(up(P->crow_ptr, P->st.row_ptr.data(), 4 * (N + 1))); HIPCHK_S(up(P->cobs, P->st.obs.data(), 4 * P->n_used)); HIPCHK_S(up(P->ctrk, P->st.trk.data(), 4 * P->n_used));
  HIPCHK_S(up(P->track_used, P->st.track_used.data(), T)); HIPCHK_S(up(P->active, P->h_active.data(), 2 * N + T));
  HIPCHK_S(up(P->intrinsics, intrinsics, 24 * N)); HIPCHK_S(up(P->cam_est, est.data(), N));
  if (int st = sync_stream(s, "full bundle adjustment problem create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

gsfm_status b6_solve_impl(gsfm_ba6_problem* P, double* rot_aa, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  if (!P || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b6_options(opt);
  gsfm_ba_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->num_observations_used = P->n_used; summary->num_active_cameras = P->st.n_active_cams; summary->num_active_points = P->st.n_active_points;
  summary->termination = GSFM_TERM_GRADIENT_TOLERANCE;
  if (P->n_used == 0) return GSFM_OK;   // nothing to adjust: nothing changes
  const double t0 = now_ms();
  const size_t N = P->n_cams, T = P->n_tracks;
  if (int st = b6_upload_point(P, rot_aa, cam_pos, points)) return (gsfm_status)st;
  if (int st = b6_lm_solve(P, o, summary)) return (gsfm_status)st;
  hvec<double> xh(3 * P->n_nodes);
  if (int st = b6_read(P, xh.data(), P->x, 24 * P->n_nodes, "download the estimates")) return (gsfm_status)st;
  // only the active nodes are parameters: every other row of the caller's arrays keeps its bytes
  for (size_t k = 0; k < N; ++k)
    if (P->h_active[k]) { std::copy(&xh[3 * k], &xh[3 * k] + 3, rot_aa + 3 * k); std::copy(&xh[3 * (N + k)], &xh[3 * (N + k)] + 3, cam_pos + 3 * k); }
  for (size_t t = 0; t < T; ++t) if (P->h_active[2 * N + t]) std::copy(&xh[3 * (2 * N + t)], &xh[3 * (2 * N + t)] + 3, points + 3 * t);
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

// node-ordered camera vector (2 N x 3) -> per camera w then o (N x 6), and back
void b6_interleave(const double* nodes, size_t N, double* out) {
  for (size_t k = 0; k < N; ++k) for (int c = 0; c < 3; ++c) { out[6 * k + c] = nodes[3 * k + c]; out[6 * k + 3 + c] = nodes[3 * (N + k) + c]; }
}

gsfm_status b6_linearize_impl(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* cost, double* grad_rot,
                              double* grad_pos, double* grad_point, double* diag_cam, double* diag_point) {
  if (!P || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = P->n_nodes;
  gsfm_ba_options o;
  gsfm_ba6_options_default(&o);
  double c = 0.0;
  if (int st = b6_setup_linearize(P, rot_aa, cam_pos, points, o, &c)) return (gsfm_status)st;
  hvec<double> g3(3 * NN), d6(6 * NN), bx(9 * N);
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g, 24 * NN, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg, 48 * NN, hipMemcpyDeviceToHost, P->mem.s));
  if (N) HIPCHK_S(hipMemcpyAsync(bx.data(), P->Bx, 72 * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearize outputs")) return (gsfm_status)st;
  if (grad_rot) std::copy(g3.begin(), g3.begin() + 3 * N, grad_rot);
  if (grad_pos) std::copy(g3.begin() + 3 * N, g3.begin() + 6 * N, grad_pos);
  if (grad_point) std::copy(g3.begin() + 6 * N, g3.end(), grad_point);
  auto sym = [&](size_t node, int r, int cc) {
    static const int idx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    return d6[6 * node + idx[r][cc]];
  };
  if (diag_cam)
    for (size_t k = 0; k < N; ++k)
      for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) {
          double* B = diag_cam + 36 * k;
          B[6 * r + cc] = sym(k, r, cc); B[6 * (3 + r) + 3 + cc] = sym(N + k, r, cc);
          B[6 * r + 3 + cc] = bx[9 * k + 3 * r + cc]; B[6 * (3 + cc) + r] = bx[9 * k + 3 * r + cc];
        }
  if (diag_point)
    for (size_t t = 0; t < T; ++t)
      for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) diag_point[9 * t + 3 * r + cc] = sym(2 * N + t, r, cc);
  if (cost) *cost = c;
  return GSFM_OK;
}

gsfm_status b6_residuals_impl(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  if (!P || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t O = P->n_obs;
  if (O == 0) return GSFM_OK;
  FlatLayout L;
  const Slot<double> r = L.take<double>(2 * O), rho = L.take<double>(O);
  DevBuf<char> scratch;
  if (scratch.alloc(L.total) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  if (int st = b6_upload_point(P, rot_aa, cam_pos, points)) return (gsfm_status)st;
  b6_cost(P, P->x, (double*)(scratch.p + r.off), (double*)(scratch.p + rho.off));
  if (r_out) HIPCHK_S(hipMemcpyAsync(r_out, scratch.p + r.off, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (rho_out) HIPCHK_S(hipMemcpyAsync(rho_out, scratch.p + rho.off, 8 * O, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "residuals");
}

gsfm_status b6_schur_matvec_impl(gsfm_ba6_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b6_options(opt);
  const size_t N = P->n_cams;
  if (N == 0) return GSFM_OK;
  hvec<double> nodes(6 * N), outn(6 * N);
  for (size_t k = 0; k < N; ++k) for (int c = 0; c < 3; ++c) { nodes[3 * k + c] = v[6 * k + c]; nodes[3 * (N + k) + c] = v[6 * k + 3 + c]; }
  b6_jacobi_scale(P, o);
  b6_prep(P, radius, o);
  HIPCHK_S(hipMemcpyAsync(P->p, nodes.data(), 48 * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_ba_scale, ba_grid(2 * N), dim3(256), 0, P->mem.s, 2 * N, P->active, P->S, P->p, 1.0, P->q);
  b6_schur_product(P, P->q, P->p, P->Ap);
  HIPCHK_S(hipMemcpyAsync(outn.data(), P->Ap, 48 * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "schur_matvec")) return (gsfm_status)st;
  b6_interleave(outn.data(), N, y);
  return GSFM_OK;
}

gsfm_status b6_step_check_impl(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, const gsfm_ba_options* opt,
                               double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out, double* delta_point_out,
                               double* jdelta_out, double* scal_out, int32_t* info_out) {
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b6_options(opt);
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs;
  DevBuf<char> scratch;
  if (jdelta_out && O > 0 && scratch.alloc(16 * O) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc J delta buffer");
  double* jd_dev = (jdelta_out && O > 0) ? (double*)scratch.p : nullptr;
  double cost = 0.0;
  if (int st = b6_setup_linearize(P, rot_aa, cam_pos, points, o, &cost)) return (gsfm_status)st;
  BaStep step;
  if (int st = b6_step(P, radius, o, &step, jd_dev)) return (gsfm_status)st;
  double hs[B6_N];
  hvec<double> rhs_n(6 * N), yc_n(6 * N);
  auto down = [&](double* dst, const double* src, size_t rows) { return (dst && rows) ? hipMemcpyAsync(dst, src, 24 * rows, hipMemcpyDeviceToHost, P->mem.s) : hipSuccess; };
  HIPCHK_S(hipMemcpyAsync(hs, P->scal, sizeof(hs), hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(down(rhs_n.data(), P->rhs, 2 * N)); HIPCHK_S(down(yc_n.data(), P->y, 2 * N)); HIPCHK_S(down(yp_out, P->y + 6 * N, T));
  HIPCHK_S(down(delta_rot_out, P->delta, N)); HIPCHK_S(down(delta_pos_out, P->delta + 3 * N, N)); HIPCHK_S(down(delta_point_out, P->delta + 6 * N, T));
  if (jd_dev) HIPCHK_S(hipMemcpyAsync(jdelta_out, jd_dev, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "step check")) return (gsfm_status)st;
  if (rhs_out) b6_interleave(rhs_n.data(), N, rhs_out);
  if (yc_out) b6_interleave(yc_n.data(), N, yc_out);
  if (scal_out) {
    scal_out[0] = -hs[B6_DG] - 0.5 * hs[B6_JD2];   // the solve's model cost change
    scal_out[1] = hs[B6_DG]; scal_out[2] = hs[B6_JD2]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.cg; info_out[1] = step.stalled ? 1 : 0; }
  return GSFM_OK;
}

gsfm_status b6_time_kernels_impl(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us) {
  DeviceGuard g(P->device);
  gsfm_ba_options o;
  gsfm_ba6_options_default(&o);
  double cost = 0.0;
  if (int st = b6_setup_linearize(P, rot_aa, cam_pos, points, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = b6_step(P, radius, o, &step)) return (gsfm_status)st;
  b6_cameras(P, P->x);       // (the step's trial cost is not evaluated here; the records are those of x)
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
  timed([&] { b6_cameras(P, P->x); });
  timed([&] { B6_TRACKS(P, k_ba6_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_lin, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), P->g, P->Dg, P->Bx); });
  timed([&] { B6_TRACKS(P, k_ba6_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { B6_TRACKS(P, k_ba6_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->q, (const double*)P->zt, 1.0, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv); });
  timed([&] { B6_TRACKS(P, k_ba6_quad_tracks, (const double*)P->delta, P->pt_scratch, (double*)nullptr); });
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return (gsfm_status)st;
}

}  // namespace

extern "C" {

int gsfm_ba6_abi_version(void) { return GSFM_BA6_ABI_VERSION; }

// gsfm_ba.h's defaults with the PCG tolerance two decades lower: see the header
void gsfm_ba6_options_default(gsfm_ba_options* o) {
  gsfm_ba_options_default(o);
  o->cg_relative_tolerance = 1e-14;
}

void gsfm_ba6_problem_destroy(gsfm_ba6_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

gsfm_status gsfm_ba6_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                                    const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba6_problem** out) {
  return guarded("full bundle adjustment problem creation", b6_create_impl, n_cams, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 point_estimated, out);
}

gsfm_status gsfm_ba6_set_loss(gsfm_ba6_problem* P, const gsfm_loss_node* prog, int32_t n) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || n > 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the full bundle adjustment takes a loss of one leaf (composite programs are not supported)");
  // Every refusal below returns before P is read or written (the ABI tests hand in a handle that is no problem at all): keep the checks
  // ahead of the first use of P.
  gsfm::DevLossNode leaf;
  std::memset(&leaf, 0, sizeof(leaf));
  leaf.kind = GSFM_LOSS_TRIVIAL;
  if (n == 1) {
    const int k = prog[0].kind;
    if (!(k == GSFM_LOSS_TRIVIAL || k == GSFM_LOSS_HUBER || k == GSFM_LOSS_SOFT_L1 || k == GSFM_LOSS_TUKEY || k == GSFM_LOSS_GEMAN_MCCLURE))
      return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "the full bundle adjustment takes the losses Trivial, Huber, SoftLOne, Tukey and GemanMcClure (MAGSAC and the other leaves are not supported)");
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

gsfm_status gsfm_ba6_solve(gsfm_ba6_problem* P, double* rot_aa, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  return guarded("the full bundle adjustment", b6_solve_impl, P, rot_aa, cam_pos, points, opt, summary);
}

gsfm_status gsfm_ba6_residuals(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  return guarded("full bundle adjustment residuals", b6_residuals_impl, P, rot_aa, cam_pos, points, r_out, rho_out);
}

gsfm_status gsfm_ba6_linearize(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* cost, double* grad_rot,
                               double* grad_pos, double* grad_point, double* diag_cam, double* diag_point) {
  return guarded("full bundle adjustment linearisation", b6_linearize_impl, P, rot_aa, cam_pos, points, cost, grad_rot, grad_pos, grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_ba6_schur_matvec(gsfm_ba6_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_ba6_linearize or gsfm_ba6_step_check first");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("full bundle adjustment Schur product", b6_schur_matvec_impl, P, v, radius, opt, y);
}

gsfm_status gsfm_ba6_step_check(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, const gsfm_ba_options* opt,
                                double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out, double* delta_point_out,
                                double* jdelta_out, double* scal_out, int32_t* info_out) {
  if (!P || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("full bundle adjustment step check", b6_step_check_impl, P, rot_aa, cam_pos, points, radius, opt, rhs_out, yc_out, yp_out, delta_rot_out,
                 delta_pos_out, delta_point_out, jdelta_out, scal_out, info_out);
}

gsfm_status gsfm_ba6_time_kernels(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, int32_t reps,
                                  double* out_us) {
  if (!P || !out_us || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  return guarded("full bundle adjustment kernel timing", b6_time_kernels_impl, P, rot_aa, cam_pos, points, radius, reps, out_us);
}

}  // extern "C"
