// Host side of camera-position estimation (include/gsfm_pos.h): problem assembly, the Levenberg-Marquardt loop with Ceres 1.14's
// TrustRegionMinimizer + LevenbergMarquardtStrategy rules (restated from oracle/ref_solver.cpp::lm_solve for Euclidean parameters), exact
// steps by the dense tiled Cholesky (solver_dense.hpp, enqueue_chol_solve) or block-Jacobi PCG.  The kernels are in pos_kernels.hpp; the
// host sequences launches and reads a few scalars per LM iteration (and one per cg_check_interval PCG iterations).
#pragma once
#include "host_common.hpp"
#include "solver_launch.hpp"
#include "solver_dense.hpp"
#include "pos_kernels.hpp"
#include "../../include/gsfm_pos.h"

struct gsfm_pos_problem {
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t n_cams = 0;
  uint64_t n_edges = 0;
  std::vector<uint8_t> present;            // camera appears in an edge
  DevBuf<uint32_t> row_ptr, nbr, eid, ei, ej;
  DevBuf<double> dir_k, dir_e, H;
  DevBuf<uint8_t> active;
  // per camera (3 or more doubles each)
  DevBuf<double> x, cand, g, Dg, S, D2, Mblk, Minv, b, r, z, p, q, y, Ap, delta, v, part, scal;
  DevBuf<double> denseA, denseL, dense_x;
  DevBuf<int> dense_info;
  // loss
  DevBuf<DevLoss> d_loss;
  DevBuf<double> tables[3];
  int lm = LM_SIMPLE;                      // kernel specialisation of the loss (LM_SIMPLE / LM_PROGRAM / POS_LM_EXT)
  gsfm_loss_callback cb = nullptr;
  void* cb_user = nullptr;
  DevBuf<double> rho_ext, s_dev;
  std::vector<double> h_s, h_rho;
  bool have_lin = false;                   // a linearisation from gsfm_pos_linearize / gsfm_pos_step_check is on the device
};

namespace {

using gsfm::PosDev;

enum { PS_RZ0 = 0, PS_RZA = 1, PS_RZB = 2, PS_PAP = 3, PS_DV = 4, PS_VV = 5, PS_STEP2 = 6, PS_DG = 7, PS_DLD = 8, PS_COST = 9, PS_GMAX = 10,
       PS_XNORM2 = 11, PS_N = 12 };

PosDev pos_dev(gsfm_pos_problem* P) {
  PosDev a{};
  a.n_cams = P->n_cams; a.n_edges = (uint32_t)P->n_edges;
  a.row_ptr = P->row_ptr.p; a.nbr = P->nbr.p; a.eid = P->eid.p; a.dir_k = P->dir_k.p; a.ei = P->ei.p; a.ej = P->ej.p; a.dir_e = P->dir_e.p;
  a.active = P->active.p; a.H = P->H.p; a.loss = P->d_loss.p; a.rho_ext = P->rho_ext.p;
  return a;
}
inline dim3 pos_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline dim3 pos_row_grid(uint32_t n_cams) { return dim3((n_cams + 3) / 4); }

int pos_sync(gsfm_pos_problem* P, const char* what) {
  const hipError_t e = hipStreamSynchronize(P->stream);
  if (e != hipSuccess) return fail(GSFM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  const hipError_t l = hipGetLastError();
  if (l != hipSuccess) return fail(GSFM_ERR_HIP, std::string(what) + " (launch): " + hipGetErrorString(l));
  return 0;
}

// scal[slot] = a . b (mask: per camera), in a fixed order
void pos_dot(gsfm_pos_problem* P, const double* a, const double* b, const uint8_t* mask, int slot) {
  hipLaunchKernelGGL(k_pos_dot, dim3(GSFM_POS_PARTS), dim3(256), 0, P->stream, a, b, mask, 3 * (size_t)P->n_cams, P->part.p);
  hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, P->stream, P->part.p, P->scal.p + slot, 0);
}

// host-callback loss: s of every edge at pos, rho from the callback (in edge order), the triples uploaded for the linearisation; returns the cost
int pos_callback_rho(gsfm_pos_problem* P, const double* pos, double* cost) {
  const PosDev a = pos_dev(P);
  hipLaunchKernelGGL(k_pos_resid, pos_grid(P->n_edges), dim3(256), 0, P->stream, a, pos, (double*)nullptr, P->s_dev.p, (double*)nullptr, 0);
  HIPCHK(hipMemcpyAsync(P->h_s.data(), P->s_dev.p, 8 * P->n_edges, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "callback residuals")) return st;
  double c = 0.0;
  for (size_t e = 0; e < P->n_edges; ++e) { P->cb(P->cb_user, P->h_s[e], &P->h_rho[3 * e]); c += 0.5 * P->h_rho[3 * e]; }
  *cost = c;
  return 0;
}

// cost of pos into scal[PS_COST] (in-kernel loss) or *cost (callback: then also the rho triples at pos are staged in h_rho)
int pos_cost(gsfm_pos_problem* P, const double* pos, double* cost) {
  if (P->cb) return pos_callback_rho(P, pos, cost);
  const PosDev a = pos_dev(P);
  if (P->lm == LM_SIMPLE) hipLaunchKernelGGL(k_pos_cost<LM_SIMPLE>, dim3(GSFM_POS_PARTS), dim3(256), 0, P->stream, a, pos, P->part.p);
  else hipLaunchKernelGGL(k_pos_cost<LM_PROGRAM>, dim3(GSFM_POS_PARTS), dim3(256), 0, P->stream, a, pos, P->part.p);
  hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, P->stream, P->part.p, P->scal.p + PS_COST, 0);
  return 0;
}

// linearisation at P->x (the callback's rho triples of x must be in h_rho)
int pos_linearize(gsfm_pos_problem* P) {
  const PosDev a = pos_dev(P);
  if (P->cb) {
    HIPCHK(hipMemcpyAsync(P->rho_ext.p, P->h_rho.data(), 24 * P->n_edges, hipMemcpyHostToDevice, P->stream));
    hipLaunchKernelGGL(k_pos_lin<POS_LM_EXT>, pos_row_grid(P->n_cams), dim3(256), 0, P->stream, a, P->x.p, P->g.p, P->Dg.p);
    return pos_sync(P, "linearisation");   // (h_rho is overwritten by the next trial point)
  }
  if (P->lm == LM_SIMPLE) hipLaunchKernelGGL(k_pos_lin<LM_SIMPLE>, pos_row_grid(P->n_cams), dim3(256), 0, P->stream, a, P->x.p, P->g.p, P->Dg.p);
  else hipLaunchKernelGGL(k_pos_lin<LM_PROGRAM>, pos_row_grid(P->n_cams), dim3(256), 0, P->stream, a, P->x.p, P->g.p, P->Dg.p);
  return 0;
}

// gradient max norm and |x| over the free parameters into scal[PS_GMAX], scal[PS_XNORM2]
void pos_norms(gsfm_pos_problem* P) {
  hipLaunchKernelGGL(k_pos_absmax, dim3(GSFM_POS_PARTS), dim3(256), 0, P->stream, P->g.p, P->active.p, 3 * (size_t)P->n_cams, P->part.p);
  hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, P->stream, P->part.p, P->scal.p + PS_GMAX, 1);
  pos_dot(P, P->x.p, P->x.p, P->active.p, PS_XNORM2);
}

// Exact step by the dense tiled Cholesky; *ok = false: not used (size, memory; *info = -1) or the factorisation met a non-positive pivot
// (*info > 0).  K_tiles (may be NULL): a host copy of the assembled tiles, taken before the factorisation overwrites them.
int pos_dense_step(gsfm_pos_problem* P, bool* ok, int* info_out, std::vector<double>* K_tiles) {
  *ok = false; *info_out = -1;
  const uint32_t n = 3 * P->n_cams, T = (n + GSFM_CB - 1) / GSFM_CB;
  if (T > GSFM_DENSE_MAX_T) return 0;
  const size_t elems = chol_num_tiles(T) * GSFM_TILE_ELEMS;
  if (!P->denseA.p) {
    if (P->denseA.alloc(elems) != hipSuccess || P->denseL.alloc(elems, true) != hipSuccess || P->dense_x.alloc((size_t)T * GSFM_CB, true) != hipSuccess ||
        P->dense_info.alloc(1) != hipSuccess) {
      P->denseA.release(); P->denseL.release(); P->dense_x.release(); (void)hipGetLastError();
      return 0;
    }
  }
  HIPCHK(hipMemsetAsync(P->denseA.p, 0, 8 * elems, P->stream));
  HIPCHK(hipMemsetAsync(P->dense_info.p, 0, sizeof(int), P->stream));
  hipLaunchKernelGGL(k_pos_dense_assemble, dim3(P->n_cams), dim3(256), 0, P->stream, pos_dev(P), P->S.p, P->Mblk.p, P->b.p, P->denseA.p, n, T);
  if (K_tiles) {
    K_tiles->resize(elems);
    HIPCHK(hipMemcpyAsync(K_tiles->data(), P->denseA.p, 8 * elems, hipMemcpyDeviceToHost, P->stream));
    if (int st = pos_sync(P, "dense assembly")) return st;
  }
  enqueue_chol_solve(P->denseA.p, P->denseL.p, P->dense_x.p, n, T, P->dense_info.p, P->stream, false);
  HIPCHK(hipMemcpyAsync(P->y.p, P->dense_x.p, 8 * (size_t)n, hipMemcpyDeviceToDevice, P->stream));
  int info = 0;
  HIPCHK(hipMemcpyAsync(&info, P->dense_info.p, sizeof(int), hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "dense step")) return st;
  *info_out = info;
  *ok = info == 0;
  return 0;
}

// PCG on (S L S + D^2) y = b from y = 0 (k_pos_prep set r, z, p, q); returns its iterations, *stalled: ended above the tolerance,
// *rel: the last relative residual read back, sqrt(r.M^-1 r / b.M^-1 b) of the recursion (0 when b = 0)
int pos_pcg(gsfm_pos_problem* P, const gsfm_pos_options& o, int* iters, bool* stalled, double* rel) {
  *iters = 0; *stalled = false; *rel = 0.0;
  const PosDev a = pos_dev(P);
  const uint32_t N = P->n_cams;
  pos_dot(P, P->r.p, P->z.p, nullptr, PS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal.p + PS_RZA, P->scal.p + PS_RZ0, 8, hipMemcpyDeviceToDevice, P->stream));
  double rz0 = 0.0;
  HIPCHK(hipMemcpyAsync(&rz0, P->scal.p + PS_RZ0, 8, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "pcg start")) return st;
  if (!(rz0 > 0.0) || !std::isfinite(rz0)) return 0;   // b = 0: y = 0 is the solution (a NaN right-hand side: the step is refused later)
  const int check = std::max(1, o.cg_check_interval);
  double best = rz0; int best_it = 0;
  int cur = PS_RZA, nxt = PS_RZB;
  int it = 0;
  while (it < o.max_cg_iterations) {
    hipLaunchKernelGGL(k_pos_matvec<true>, pos_row_grid(N), dim3(256), 0, P->stream, a, P->q.p, P->p.p, P->S.p, P->D2.p, P->Ap.p);
    pos_dot(P, P->p.p, P->Ap.p, nullptr, PS_PAP);
    hipLaunchKernelGGL(k_pos_pcg_update, pos_grid(N), dim3(256), 0, P->stream, N, P->scal.p, cur, PS_PAP, P->p.p, P->Ap.p, P->y.p, P->r.p, P->z.p, P->Minv.p);
    pos_dot(P, P->r.p, P->z.p, nullptr, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, pos_grid(N), dim3(256), 0, P->stream, N, P->scal.p, nxt, cur, P->active.p, P->S.p, P->z.p, P->p.p, P->q.p);
    std::swap(cur, nxt);
    ++it;
    if (it % check == 0 || it == o.max_cg_iterations) {
      double rz = 0.0;
      HIPCHK(hipMemcpyAsync(&rz, P->scal.p + cur, 8, hipMemcpyDeviceToHost, P->stream));
      if (int st = pos_sync(P, "pcg")) return st;
      *rel = std::sqrt(std::fmax(rz, 0.0) / rz0);
      if (!std::isfinite(rz)) { *rel = rz; break; }
      if (*rel <= o.cg_relative_tolerance) { *iters = it; return 0; }
      if (rz <= 0.25 * best) { best = rz; best_it = it; }   // the relative residual sqrt(rz / rz0) halved
      else if (o.cg_stall_iterations > 0 && it - best_it >= o.cg_stall_iterations) break;
    }
  }
  *iters = it;
  *stalled = true;
  return 0;
}

// One LM step's linear algebra at P->x, after its linearisation and with the Jacobi scale S in place -- shared by the solve and by
// gsfm_pos_step_check, so that the check runs the solve's own code.  LevenbergMarquardtStrategy::ComputeStep: (J^T J + D^2) y = J^T r
// in scaled coordinates, D = sqrt(clamp(diag) / radius), step = -S y; the dense Cholesky up to dense_max_cams cameras (PCG when it is
// not used or meets a non-positive pivot), then the step's scale-gauge part removed, the trial point P->cand, and scal[PS_STEP2],
// scal[PS_DG] = delta.g and scal[PS_DLD] = delta^T L delta, enqueued (the caller reads them back).  K_tiles: see pos_dense_step.
struct PosStep { bool dense = false; int info = -1; int cg = 0; bool stalled = false; double cg_rel = 0.0; };
int pos_step(gsfm_pos_problem* P, int32_t fixed, double radius, const gsfm_pos_options& o, PosStep* out, std::vector<double>* K_tiles) {
  const uint32_t N = P->n_cams;
  const PosDev a = pos_dev(P);
  *out = PosStep();
  hipLaunchKernelGGL(k_pos_prep, pos_grid(N), dim3(256), 0, P->stream, N, P->active.p, P->Dg.p, P->g.p, P->S.p, radius, o.min_lm_diagonal, o.max_lm_diagonal,
                     P->D2.p, P->Mblk.p, P->Minv.p, P->b.p, P->r.p, P->z.p, P->p.p, P->q.p, P->y.p);
  bool solved = false;
  if ((int64_t)N <= (int64_t)o.dense_max_cams) {
    if (int st = pos_dense_step(P, &solved, &out->info, K_tiles)) return st;
    if (!solved)
      hipLaunchKernelGGL(k_pos_prep, pos_grid(N), dim3(256), 0, P->stream, N, P->active.p, P->Dg.p, P->g.p, P->S.p, radius, o.min_lm_diagonal, o.max_lm_diagonal,
                         P->D2.p, P->Mblk.p, P->Minv.p, P->b.p, P->r.p, P->z.p, P->p.p, P->q.p, P->y.p);
  }
  out->dense = solved;
  if (!solved)
    if (int st = pos_pcg(P, o, &out->cg, &out->stalled, &out->cg_rel)) return st;
  // the step, its scale-gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_pos_step, pos_grid(N), dim3(256), 0, P->stream, N, P->active.p, P->S.p, P->y.p, P->x.p, fixed, o.remove_scale_gauge, P->delta.p, P->v.p);
  pos_dot(P, P->delta.p, P->v.p, nullptr, PS_DV);
  pos_dot(P, P->v.p, P->v.p, nullptr, PS_VV);
  hipLaunchKernelGGL(k_pos_project, pos_grid(N), dim3(256), 0, P->stream, N, P->scal.p, PS_DV, PS_VV, P->v.p, P->delta.p, P->x.p, P->cand.p);
  pos_dot(P, P->delta.p, P->delta.p, nullptr, PS_STEP2);
  pos_dot(P, P->delta.p, P->g.p, nullptr, PS_DG);
  hipLaunchKernelGGL(k_pos_matvec<false>, pos_row_grid(N), dim3(256), 0, P->stream, a, P->delta.p, P->delta.p, P->S.p, P->D2.p, P->Ap.p);
  pos_dot(P, P->delta.p, P->Ap.p, nullptr, PS_DLD);
  return 0;
}

int pos_lm_solve(gsfm_pos_problem* P, int32_t fixed, const gsfm_pos_options& o, gsfm_pos_summary* sum) {
  const uint32_t N = P->n_cams;
  double radius = o.initial_trust_region_radius, decrease_factor = 2.0;
  int num_invalid = 0, iteration = 0;
  double x_cost = 0.0, x_norm = 0.0, gmax = 0.0;
  double hs[PS_N];
  sum->max_radius = radius;

  auto read_scal = [&](const char* what) -> int {
    HIPCHK(hipMemcpyAsync(hs, P->scal.p, sizeof(hs), hipMemcpyDeviceToHost, P->stream));
    return pos_sync(P, what);
  };
  auto finish = [&](int term) {
    sum->termination = term; sum->num_iterations = iteration; sum->final_cost = x_cost;
    sum->final_gradient_max_norm = gmax; sum->final_radius = radius;
    if (!std::isfinite(x_cost)) sum->nonfinite = 1;
    return 0;
  };
  auto log = [&](double cost_change, double step_norm, double rel_dec, int cg) {
    if (o.verbose) fprintf(stderr, "[gsfm pos] it %3d cost %.12e dcost %.3e |g| %.3e |dx| %.3e rho %.3e radius %.3e cg %d\n",
                           iteration, x_cost, cost_change, gmax, step_norm, rel_dec, radius, cg);
  };

  // iteration 0: cost, linearisation (with the Jacobi scale of the start point), gradient norm
  double cb_cost = 0.0;
  if (int st = pos_cost(P, P->x.p, &cb_cost)) return st;
  if (int st = pos_linearize(P)) return st;
  hipLaunchKernelGGL(k_pos_scale, pos_grid(N), dim3(256), 0, P->stream, N, P->Dg.p, P->S.p, o.jacobi_scaling);
  pos_norms(P);
  if (int st = read_scal("start point")) return st;
  x_cost = P->cb ? cb_cost : hs[PS_COST];
  gmax = hs[PS_GMAX]; x_norm = std::sqrt(hs[PS_XNORM2]);
  sum->num_residual_sweeps++; sum->num_linearizations++;
  sum->initial_cost = x_cost;
  log(0, 0, 0, 0);
  if (!std::isfinite(x_cost)) return finish(GSFM_TERM_FAILURE);
  if (gmax <= o.gradient_tolerance) return finish(GSFM_TERM_GRADIENT_TOLERANCE);
  bool last_successful = false;
  while (true) {
    if (iteration >= o.max_num_iterations) return finish(GSFM_TERM_NO_CONVERGENCE);
    if (last_successful && gmax <= o.gradient_tolerance) return finish(GSFM_TERM_GRADIENT_TOLERANCE);
    if (radius <= o.min_trust_region_radius) return finish(GSFM_TERM_FAILURE);
    ++iteration;
    last_successful = false;
    PosStep step;
    if (int st = pos_step(P, fixed, radius, o, &step, nullptr)) return st;
    const int cg = step.cg;
    if (step.dense) sum->num_dense_solves++;
    else {
      sum->num_cg_iterations += cg;
      if (step.stalled) sum->num_pcg_stalled_steps++;
    }
    if (int st = read_scal("step")) return st;
    const double step2 = hs[PS_STEP2];
    bool valid = std::isfinite(step2) && std::isfinite(hs[PS_DG]) && std::isfinite(hs[PS_DLD]);
    // model cost change -(J delta)^T (r + J delta / 2) = -delta.g - delta^T L delta / 2
    const double model_cost_change = -hs[PS_DG] - 0.5 * hs[PS_DLD];
    if (valid && !(model_cost_change > 0.0)) valid = false;
    if (!valid) {   // HandleInvalidStep
      if (++num_invalid >= 5) return finish(GSFM_TERM_FAILURE);
      radius /= decrease_factor; decrease_factor *= 2.0;
      sum->num_unsuccessful_steps++;
      log(0, 0, 0, cg);
      continue;
    }
    num_invalid = 0;
    double cand_cost = 0.0;
    if (int st = pos_cost(P, P->cand.p, &cand_cost)) return st;
    if (!P->cb) {
      HIPCHK(hipMemcpyAsync(&cand_cost, P->scal.p + PS_COST, 8, hipMemcpyDeviceToHost, P->stream));
      if (int st = pos_sync(P, "trial cost")) return st;
    }
    sum->num_residual_sweeps++;
    if (!std::isfinite(cand_cost)) { cand_cost = std::numeric_limits<double>::max(); sum->nonfinite = 1; }
    const double step_norm = std::sqrt(step2);
    const double cost_change = x_cost - cand_cost;
    const double rel_dec = cost_change / model_cost_change;
    if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { log(cost_change, step_norm, rel_dec, cg); return finish(GSFM_TERM_PARAMETER_TOLERANCE); }
    if (std::fabs(cost_change) <= o.function_tolerance * x_cost) { log(cost_change, step_norm, rel_dec, cg); return finish(GSFM_TERM_FUNCTION_TOLERANCE); }
    if (rel_dec > o.min_relative_decrease) {   // HandleSuccessfulStep
      HIPCHK(hipMemcpyAsync(P->x.p, P->cand.p, 24 * (size_t)N, hipMemcpyDeviceToDevice, P->stream));
      x_cost = cand_cost;
      if (int st = pos_linearize(P)) return st;
      pos_norms(P);
      if (int st = read_scal("linearisation")) return st;
      gmax = hs[PS_GMAX]; x_norm = std::sqrt(hs[PS_XNORM2]);
      sum->num_linearizations++;
      radius = radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rel_dec - 1.0, 3));
      radius = std::fmin(o.max_trust_region_radius, radius);
      decrease_factor = 2.0;
      sum->num_successful_steps++;
      last_successful = true;
    } else {   // HandleUnsuccessfulStep
      radius /= decrease_factor; decrease_factor *= 2.0;
      sum->num_unsuccessful_steps++;
    }
    sum->max_radius = std::fmax(sum->max_radius, radius);
    log(cost_change, step_norm, rel_dec, cg);
  }
}

// The active set (the present cameras, less fixed_cam when >= 0), x = pos, the cost and the linearisation at x: what a solve does before
// its first step.  *cost: the cost of pos.
int pos_setup_linearize(gsfm_pos_problem* P, const double* pos, int32_t fixed_cam, double* cost) {
  std::vector<uint8_t> act(P->present);
  if (fixed_cam >= 0) act[fixed_cam] = 0;
  HIPCHK(hipMemcpyAsync(P->active.p, act.data(), act.size(), hipMemcpyHostToDevice, P->stream));
  HIPCHK(hipMemcpyAsync(P->x.p, pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->stream));
  double cb_cost = 0.0;
  if (int st = pos_cost(P, P->x.p, &cb_cost)) return st;
  if (int st = pos_linearize(P)) return st;
  double c = cb_cost;
  if (!P->cb) HIPCHK(hipMemcpyAsync(&c, P->scal.p + PS_COST, 8, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "linearisation")) return st;
  *cost = c;
  P->have_lin = true;
  return 0;
}

int pos_create_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
                    gsfm_pos_problem** out, gsfm_pos_problem** live) {
  if (!out) return fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (n_cams == 0 || n_edges == 0) return fail(GSFM_ERR_EMPTY, "no cameras or no edges");
  if (!edge_i || !edge_j || !rel_t || !rot_aa) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31) || n_cams >= (1u << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges or cameras)");
  for (uint64_t e = 0; e < n_edges; ++e)
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams || edge_i[e] == edge_j[e]) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has a bad camera index");
  if (const char* why = no_device_reason("gsfm_pos_problem_create")) return fail(GSFM_ERR_NO_DEVICE, why);
  const size_t N = n_cams, E = n_edges, ND = 2 * E;
  // device memory: entries 4 + 4 + 24 + 48 B, edges 4 + 4 + 24 B, cameras ~ 60 doubles, the E x 3 upload of the directions
  const double need = (double)ND * 80 + (double)E * (32 + 24 + 24) + (double)N * 8 * 64 + (double)(N + 1) * 4;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b < need * 1.05 + (64u << 20))
    return fail(GSFM_ERR_HIP, "not enough free device memory for the position problem (" + std::to_string((long long)(need / 1048576)) + " MiB needed, " +
                std::to_string((long long)(free_b / 1048576)) + " MiB free)");
  (void)hipGetLastError();
  gsfm_pos_problem* P = new gsfm_pos_problem;
  *live = P;
  (void)hipGetDevice(&P->device);
  P->n_cams = n_cams; P->n_edges = n_edges;
  // CSR of directed entries: counting sort by neighbour, then a stable one by row -> neighbours sorted within a row, ties in edge order
  std::vector<uint32_t> cnt(N + 1, 0);
  for (size_t e = 0; e < E; ++e) { cnt[edge_i[e] + 1]++; cnt[edge_j[e] + 1]++; }
  for (size_t k = 0; k < N; ++k) cnt[k + 1] += cnt[k];
  std::vector<uint32_t> row_ptr(cnt);
  std::vector<uint32_t> by_nbr(ND);   // directed entry id u = 2 e + side (side 1: the j-end's entry), sorted by neighbour
  {
    std::vector<uint32_t> pos(cnt.begin(), cnt.end() - 1);
    for (size_t e = 0; e < E; ++e) { by_nbr[pos[edge_j[e]]++] = (uint32_t)(2 * e); by_nbr[pos[edge_i[e]]++] = (uint32_t)(2 * e + 1); }
  }
  hvec<uint32_t> nbr(ND), eid(ND), pos_i(E), pos_j(E);
  {
    std::vector<uint32_t> pos(row_ptr.begin(), row_ptr.end() - 1);
    for (size_t t = 0; t < ND; ++t) {
      const uint32_t u = by_nbr[t], e = u >> 1, side = u & 1;
      const uint32_t row = side ? edge_j[e] : edge_i[e], m = side ? edge_i[e] : edge_j[e];
      const uint32_t d = pos[row]++;
      nbr[d] = m; eid[d] = e;
      (side ? pos_j : pos_i)[e] = d;
    }
  }
  P->present.assign(N, 0);
  for (size_t k = 0; k < N; ++k) P->present[k] = row_ptr[k + 1] > row_ptr[k];
  if (hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking) != hipSuccess) return fail(GSFM_ERR_HIP, "hipStreamCreate failed");
  bool ok = P->row_ptr.upload(row_ptr) == hipSuccess && P->nbr.upload(nbr) == hipSuccess && P->eid.upload(eid) == hipSuccess &&
            P->dir_k.alloc(3 * ND) == hipSuccess && P->dir_e.alloc(3 * E) == hipSuccess &&
            P->H.alloc(6 * ND) == hipSuccess && P->active.alloc(N, true) == hipSuccess && P->scal.alloc(PS_N, true) == hipSuccess &&
            P->part.alloc(GSFM_POS_PARTS) == hipSuccess && P->d_loss.alloc(1) == hipSuccess;
  DevBuf<double>* vecs3[] = {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->r, &P->z, &P->p, &P->q, &P->y, &P->Ap, &P->delta, &P->v};
  for (DevBuf<double>* v : vecs3) ok = ok && v->alloc(3 * N, true) == hipSuccess;
  ok = ok && P->Dg.alloc(6 * N, true) == hipSuccess && P->Mblk.alloc(6 * N) == hipSuccess && P->Minv.alloc(9 * N) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return fail(GSFM_ERR_HIP, "allocating the position problem failed"); }
  DevBuf<uint32_t> d_pos_i, d_pos_j;
  DevBuf<double> d_rel, d_rot;
  std::vector<double> rel(rel_t, rel_t + 3 * E), rot(rot_aa, rot_aa + 3 * N);
  if (P->ei.alloc(E) != hipSuccess || hipMemcpy(P->ei.p, edge_i, 4 * E, hipMemcpyHostToDevice) != hipSuccess ||
      P->ej.alloc(E) != hipSuccess || hipMemcpy(P->ej.p, edge_j, 4 * E, hipMemcpyHostToDevice) != hipSuccess ||
      d_pos_i.upload(pos_i) != hipSuccess || d_pos_j.upload(pos_j) != hipSuccess || d_rel.upload(rel) != hipSuccess || d_rot.upload(rot) != hipSuccess)
    return fail(GSFM_ERR_HIP, "uploading the position problem failed");
  hipLaunchKernelGGL(k_pos_directions, pos_grid(E), dim3(256), 0, P->stream, (uint32_t)E, P->ei.p, d_rot.p, d_rel.p, d_pos_i.p, d_pos_j.p, P->dir_e.p, P->dir_k.p);
  // default loss: Ceres' NULL loss (the estimator layer sets the reference's HuberLoss(0.1))
  DevLoss L; std::memset(&L, 0, sizeof(L));
  HIPCHK(hipMemcpy(P->d_loss.p, &L, sizeof(L), hipMemcpyHostToDevice));
  if (int st = pos_sync(P, "position problem create")) return st;
  *out = P;
  *live = nullptr;
  return 0;
}

}  // namespace

extern "C" {

int gsfm_pos_abi_version(void) { return GSFM_POS_ABI_VERSION; }

void gsfm_pos_options_default(gsfm_pos_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 400; o->jacobi_scaling = 1;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
  o->dense_max_cams = 1000; o->max_cg_iterations = 2000; o->cg_relative_tolerance = 1e-12; o->cg_check_interval = 8; o->cg_stall_iterations = 200;
  o->remove_scale_gauge = 1; o->verbose = 0;
}

void gsfm_pos_problem_destroy(gsfm_pos_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->stream) { (void)hipStreamSynchronize(P->stream); (void)hipStreamDestroy(P->stream); }
  delete P;
}

gsfm_status gsfm_pos_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                    const double* rot_aa, gsfm_pos_problem** out) {
  gsfm_pos_problem* live = nullptr;
  int st;
  try {
    st = pos_create_impl(n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa, out, &live);
  } catch (const std::exception& e) {
    st = fail(GSFM_ERR_INVALID_ARG, std::string("position problem creation ran out of host resources: ") + e.what());
  }
  if (st && live) { gsfm_pos_problem_destroy(live); if (out) *out = nullptr; }
  return (gsfm_status)st;
}

gsfm_status gsfm_pos_set_loss(gsfm_pos_problem* P, const gsfm_loss_node* prog, int32_t n) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  DevLoss L;
  if (int st = build_dev_loss(prog, n, P->tables, L)) return (gsfm_status)st;
  bool simple = n == 0;
  if (n == 1) {
    const int k = prog[0].kind;
    simple = k == GSFM_LOSS_TRIVIAL || k == GSFM_LOSS_HUBER || k == GSFM_LOSS_SOFT_L1 || k == GSFM_LOSS_TUKEY || k == GSFM_LOSS_GEMAN_MCCLURE;
  }
  P->lm = simple ? LM_SIMPLE : LM_PROGRAM;
  P->cb = nullptr;
  HIPCHK_S(hipMemcpy(P->d_loss.p, &L, sizeof(L), hipMemcpyHostToDevice));
  return GSFM_OK;
}

gsfm_status gsfm_pos_set_loss_callback(gsfm_pos_problem* P, gsfm_loss_callback fn, void* user) {
  if (!P || !fn) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  if (!P->rho_ext.p && (P->rho_ext.alloc(3 * P->n_edges) != hipSuccess || P->s_dev.alloc(P->n_edges) != hipSuccess))
    return (gsfm_status)fail(GSFM_ERR_HIP, "allocating callback-loss buffers failed");
  P->h_s.resize(P->n_edges); P->h_rho.resize(3 * P->n_edges);
  P->cb = fn; P->cb_user = user;
  return GSFM_OK;
}

gsfm_status gsfm_pos_solve(gsfm_pos_problem* P, double* pos, int32_t fixed_cam, const gsfm_pos_options* opt, gsfm_pos_summary* summary) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (fixed_cam < -1 || fixed_cam >= (int64_t)P->n_cams || (fixed_cam >= 0 && !P->present[fixed_cam]))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "fixed_cam must be -1 or a camera that appears in an edge");
  DeviceGuard g(P->device);
  gsfm_pos_options o;
  if (opt) o = *opt; else gsfm_pos_options_default(&o);
  gsfm_pos_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->num_edges_used = P->n_edges;
  const double t0 = now_ms();
  std::vector<uint8_t> act(P->present);
  if (fixed_cam >= 0) act[fixed_cam] = 0;
  HIPCHK_S(hipMemcpyAsync(P->active.p, act.data(), act.size(), hipMemcpyHostToDevice, P->stream));
  HIPCHK_S(hipMemcpyAsync(P->x.p, pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->stream));
  if (int st = pos_lm_solve(P, fixed_cam, o, summary)) return (gsfm_status)st;
  HIPCHK_S(hipMemcpyAsync(pos, P->x.p, 24 * (size_t)P->n_cams, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "download positions")) return (gsfm_status)st;
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status gsfm_pos_residuals(gsfm_pos_problem* P, const double* pos, double* r_out, double* rho_out) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t E = P->n_edges;
  DevBuf<double> d_r, d_rho, d_s;
  if (d_r.alloc(3 * E) != hipSuccess || d_rho.alloc(E) != hipSuccess || d_s.alloc(E) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  HIPCHK_S(hipMemcpyAsync(P->cand.p, pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->stream));
  hipLaunchKernelGGL(k_pos_resid, pos_grid(E), dim3(256), 0, P->stream, pos_dev(P), P->cand.p, d_r.p, d_s.p, d_rho.p, P->cb ? 0 : 1);
  std::vector<double> s(E);
  if (r_out) HIPCHK_S(hipMemcpyAsync(r_out, d_r.p, 24 * E, hipMemcpyDeviceToHost, P->stream));
  if (rho_out && !P->cb) HIPCHK_S(hipMemcpyAsync(rho_out, d_rho.p, 8 * E, hipMemcpyDeviceToHost, P->stream));
  HIPCHK_S(hipMemcpyAsync(s.data(), d_s.p, 8 * E, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "residuals")) return (gsfm_status)st;
  if (rho_out && P->cb) for (size_t e = 0; e < E; ++e) { double t[3]; P->cb(P->cb_user, s[e], t); rho_out[e] = t[0]; }
  return GSFM_OK;
}

gsfm_status gsfm_pos_linearize(gsfm_pos_problem* P, const double* pos, double* gradient, double* diag_blocks, double* cost) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams;
  double c = 0.0;
  if (int st = pos_setup_linearize(P, pos, -1, &c)) return (gsfm_status)st;
  std::vector<double> g3(3 * N), d6(6 * N);
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g.p, 24 * N, hipMemcpyDeviceToHost, P->stream));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg.p, 48 * N, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "linearize outputs")) return (gsfm_status)st;
  if (gradient) std::copy(g3.begin(), g3.end(), gradient);
  if (diag_blocks)
    for (size_t k = 0; k < N; ++k) {
      const double* m = &d6[6 * k];
      const double full[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
      std::copy(full, full + 9, diag_blocks + 9 * k);
    }
  if (cost) *cost = c;
  return GSFM_OK;
}

gsfm_status gsfm_pos_normal_matvec(gsfm_pos_problem* P, const double* v, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_pos_linearize or gsfm_pos_step_check first");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams;
  HIPCHK_S(hipMemcpyAsync(P->q.p, v, 24 * N, hipMemcpyHostToDevice, P->stream));
  hipLaunchKernelGGL(k_pos_matvec<false>, pos_row_grid(P->n_cams), dim3(256), 0, P->stream, pos_dev(P), P->q.p, P->q.p, P->S.p, P->D2.p, P->Ap.p);
  HIPCHK_S(hipMemcpyAsync(y, P->Ap.p, 24 * N, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "normal_matvec")) return (gsfm_status)st;
  return GSFM_OK;
}

gsfm_status gsfm_pos_step_check(gsfm_pos_problem* P, const double* pos, int32_t fixed_cam, double radius, const gsfm_pos_options* opt, double* K_out,
                                double* b_out, double* y_out, double* delta_out, double* scal_out, int32_t* info_out) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (fixed_cam < -1 || fixed_cam >= (int64_t)P->n_cams || (fixed_cam >= 0 && !P->present[fixed_cam]))
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "fixed_cam must be -1 or a camera that appears in an edge");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  gsfm_pos_options o;
  if (opt) o = *opt; else gsfm_pos_options_default(&o);
  const uint32_t N = P->n_cams, n = 3 * N;
  double cost = 0.0;
  if (int st = pos_setup_linearize(P, pos, fixed_cam, &cost)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_pos_scale, pos_grid(N), dim3(256), 0, P->stream, N, P->Dg.p, P->S.p, o.jacobi_scaling);
  PosStep step;
  std::vector<double> tiles;
  if (int st = pos_step(P, fixed_cam, radius, o, &step, K_out ? &tiles : nullptr)) return (gsfm_status)st;
  double hs[PS_N];
  HIPCHK_S(hipMemcpyAsync(hs, P->scal.p, sizeof(hs), hipMemcpyDeviceToHost, P->stream));
  if (b_out) HIPCHK_S(hipMemcpyAsync(b_out, P->b.p, 8 * (size_t)n, hipMemcpyDeviceToHost, P->stream));
  if (y_out) HIPCHK_S(hipMemcpyAsync(y_out, P->y.p, 8 * (size_t)n, hipMemcpyDeviceToHost, P->stream));
  if (delta_out) HIPCHK_S(hipMemcpyAsync(delta_out, P->delta.p, 8 * (size_t)n, hipMemcpyDeviceToHost, P->stream));
  if (int st = pos_sync(P, "step check")) return (gsfm_status)st;
  if (K_out && !tiles.empty()) {
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t c = 0; c <= r; ++c) {
        const double v = tiles[chol_tile_off(r / GSFM_CB, c / GSFM_CB) + (r % GSFM_CB) * GSFM_CB + c % GSFM_CB];
        K_out[(size_t)r * n + c] = v;
        K_out[(size_t)c * n + r] = v;
      }
  }
  if (scal_out) {
    scal_out[0] = -hs[PS_DG] - 0.5 * hs[PS_DLD];   // the solve's model cost change
    scal_out[1] = hs[PS_DG]; scal_out[2] = hs[PS_DLD]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.dense ? 0 : 1; info_out[1] = step.info; info_out[2] = step.cg; }
  return GSFM_OK;
}

}  // extern "C"
