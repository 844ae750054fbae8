// Host side of the full bundle adjustment with free focal lengths (include/gsfm_ba7.h): orientations, positions, focal lengths and points,
// on the pattern of solver_ba6.hpp.  The problem's common part, the Levenberg-Marquardt operations, solve, residuals and timing are
// solver_ba.hpp's, the gauge solve and the options are solver_ba6.hpp's; here are the launches of ba7_kernels.hpp, the Schur-complement PCG
// over the cameras' 3 N nodes and the step.
// The unknowns are one array of (3 n_cams + n_tracks) x 3: angle-axis vectors, centres, intrinsics nodes (f, 0, 0), points.  A camera counts
// as three nodes; the intrinsics node's active byte is `camera active && focal_free` (ba7_kernels.hpp states the invariant on its padding).
#pragma once
#include "solver_ba6.hpp"
#include "ba7_kernels.hpp"
#include "../../include/gsfm_ba7.h"

struct gsfm_ba7_problem : BaProblem {
  uint8_t *cam_est = nullptr, *centroid_mask = nullptr;   // centroid_mask: `active` from the centres on with zeros on the intrinsics nodes
  double *intrinsics = nullptr, *Jt = nullptr, *Rt = nullptr, *Jc = nullptr, *Bx = nullptr, *gpart = nullptr;
  void cost(const double* at, double* r_out, double* rho_out) override;
  void linearize() override;
  int step(double radius, const gsfm_ba_options& o, BaStep* out) override;
};

namespace {

using gsfm::Ba7Dev;

Ba7Dev b7_dev(const gsfm_ba7_problem* P) {
  Ba7Dev a{};
  a.b = ba_dev_shared(P);
  a.Jt = P->Jt; a.Rt = P->Rt; a.Jc = P->Jc;
  return a;
}
#define B7_TRACKS(P, K, ...) ba_tracks(P, b7_dev(P), K<4>, K<16>, K<64>, __VA_ARGS__)

// the camera records (R, f, J_l) of the point `at`
void b7_cameras(gsfm_ba7_problem* P, const double* at) {
  if (P->n_cams) hipLaunchKernelGGL(k_ba7_cameras, ba_grid(P->n_cams), dim3(256), 0, P->mem.s, P->n_cams, at, (const double*)P->intrinsics, (const uint8_t*)P->cam_est, P->cams);
}
void b7_cost(gsfm_ba7_problem* P, const double* at, double* r_out = nullptr, double* rho_out = nullptr) {
  b7_cameras(P, at);
  B7_TRACKS(P, k_ba7_cost_tracks, at, P->pt_scratch, r_out, rho_out);
  ba_sum(P, P->pt_scratch, P->n_tracks, BS_COST);
}
void b7_linearize(gsfm_ba7_problem* P) {
  b7_cameras(P, P->x);
  B7_TRACKS(P, k_ba7_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(k_ba7_cam_lin, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, b7_dev(P), P->g, P->Dg, P->Bx);
}
void b7_prep(gsfm_ba7_problem* P, double radius, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_ba_prep_nodes, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, P->n_nodes, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal,
                     o.max_lm_diagonal, P->D2, P->b);
  // (the points are the nodes from 3 n_cams on)
  hipLaunchKernelGGL(k_ba6_prep_points, ba_grid(P->n_tracks), dim3(256), 0, P->mem.s, 3 * P->n_cams, P->n_tracks, P->active, P->Dg, P->S, P->D2, P->b, P->Cinv,
                     P->Gt, P->zt);
}
void b7_schur_product(gsfm_ba7_problem* P, const double* qvec, const double* pvec, double* out) {
  B7_TRACKS(P, k_ba7_point_pass, qvec, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1);
  hipLaunchKernelGGL(k_ba7_cam_pass, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, b7_dev(P), qvec, (const double*)P->zt, 1.0, pvec, (const double*)P->S,
                     (const double*)P->D2, (const double*)nullptr, out, 1);
}

// PCG on Sc y_c = rhs from y_c = 0 (k_ba7_pcg_init set r, z, p, q) over the cameras' 3 N nodes: lm_loop.hpp's driver, with the breakdown rule
int b7_pcg(gsfm_ba7_problem* P, const gsfm_ba_options& o, BaStep* out) {
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams, N3 = 3 * N;
  V.dot(P->r, P->z, nullptr, N3, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    b7_schur_product(P, P->q, P->p, P->Ap);
    V.dot(P->p, P->Ap, nullptr, N3, BS_PAP);
    hipLaunchKernelGGL(k_ba7_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, N3, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N3), dim3(256), 0, P->mem.s, N3, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, true, iterate, V.pcg_reader(), &out->cg, &out->stalled, &out->cg_rel);
}

// One LM step's linear algebra at P->x: b6_step over three nodes per camera
int b7_step(gsfm_ba7_problem* P, double radius, const gsfm_ba_options& o, BaStep* out, double* jd_out = nullptr) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes, N3 = 3 * (size_t)N;
  const DevScalars V = P->vec();
  *out = BaStep();
  b7_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_ba7_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b7_dev(P), (const double*)nullptr, (const double*)P->zt, -1.0, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_ba7_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b7_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv);
  hipLaunchKernelGGL(k_ba7_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = b7_pcg(P, o, out)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N3), dim3(256), 0, P->mem.s, N3, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) B7_TRACKS(P, k_ba7_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->b, -1.0, P->y + 3 * N3, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  const bool project = o.remove_gauge && P->n_active > 0;
  const double inv_count = P->n_active > 0 ? 1.0 / (double)P->n_active : 0.0;
  if (project) {
    for (int c = 0; c < 3; ++c) {   // the centroid of the active centres and points: the intrinsics nodes between them are masked out
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)(P->x + 3 * (size_t)N), (const uint8_t*)P->centroid_mask, 2 * (size_t)N + T, c, P->part);
      V.reduce(BS_SUMX + c);
    }
    hipLaunchKernelGGL(k_ba7_gauge_dots, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->delta,
                       (const double*)P->scal, (int)BS_SUMX, inv_count, P->gpart);
    hipLaunchKernelGGL(k_ba6_gauge_reduce, dim3(GSFM_BA6_GDOTS), dim3(256), 0, P->mem.s, (const double*)P->gpart, P->scal + B6_GRAM);
    double dots[GSFM_BA6_GDOTS], coef[GSFM_BA6_GAUGE];
    if (int st = V.read(dots, P->scal + B6_GRAM, sizeof(dots), "gauge dots")) return st;
    b6_gauge_solve(dots, coef);
    HIPCHK(hipMemcpyAsync(P->scal + B6_COEF, coef, sizeof(coef), hipMemcpyHostToDevice, P->mem.s));
    if (int st = sync_stream(P->mem.s, "gauge coefficients")) return st;   // (coef is a local)
  }
  hipLaunchKernelGGL(k_ba7_gauge_apply, ba_grid(NN), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->scal, (int)BS_SUMX, inv_count,
                     (int)B6_COEF, project ? 1 : 0, P->delta, P->cand);
  V.dot(P->delta, P->delta, nullptr, NN, BS_STEP2);
  V.dot(P->delta, P->g, nullptr, NN, BS_DG);
  B7_TRACKS(P, k_ba7_quad_tracks, (const double*)P->delta, P->pt_scratch, jd_out);
  ba_sum(P, P->pt_scratch, T, B6_JD2);
  return 0;
}

gsfm_ba_options b7_options(const gsfm_ba_options* opt) { return ba_options(opt, gsfm_ba7_options_default); }

bool b7_needs_points(const gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points) {
  return (P->n_cams > 0 && (!rot_aa || !cam_pos || !focal)) || (P->n_tracks > 0 && !points);
}
// NULL arguments and the focal lengths of the active cameras, before any device call
int b7_check_point(const gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points) {
  if (!P || b7_needs_points(P, rot_aa, cam_pos, focal, points)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  for (size_t k = 0; k < P->n_cams; ++k)
    if (P->h_active[k] && !(std::isfinite(focal[k]) && focal[k] > 0.0)) return fail(GSFM_ERR_INVALID_ARG, "the focal length of an active camera must be finite and positive");
  return 0;
}

// x = (rot_aa, cam_pos, (f, 0, 0), points), enqueued; stage must outlive the stream's copy of it (the callers wait before they return)
int b7_upload_point(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, hvec<double>* stage) {
  const size_t N = P->n_cams;
  if (N) {
    stage->assign(3 * N, 0.0);
    for (size_t k = 0; k < N; ++k) (*stage)[3 * k] = focal[k];
    HIPCHK(hipMemcpyAsync(P->x, rot_aa, 24 * N, hipMemcpyHostToDevice, P->mem.s));
    HIPCHK(hipMemcpyAsync(P->x + 3 * N, cam_pos, 24 * N, hipMemcpyHostToDevice, P->mem.s));
    HIPCHK(hipMemcpyAsync(P->x + 6 * N, stage->data(), 24 * N, hipMemcpyHostToDevice, P->mem.s));
  }
  if (P->n_tracks) HIPCHK(hipMemcpyAsync(P->x + 9 * N, points, 24 * (size_t)P->n_tracks, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}

FlatLayout b7_place(gsfm_ba7_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  SlabTake take{FlatLayout(), slab};
  take(P->scal, B6_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 9 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Bx, GSFM_BA7_BX * N);
  *zeroed = take.L.total;
  take(P->Minv, 49 * N); take(P->Cinv, 18 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS); take(P->gpart, (size_t)GSFM_BA6_GDOTS * GSFM_POS_PARTS);
  take(P->cams, GSFM_BA6_CAM_DOUBLES * N); take(P->intrinsics, 3 * N); take(P->Jt, GSFM_BA7_J * O); take(P->Rt, 2 * O); take(P->Jc, GSFM_BA7_J * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN); take(P->cam_est, N); take(P->centroid_mask, 2 * N + T);
  return take.L;
}

gsfm_status b7_create_impl(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, const uint8_t* focal_free, uint64_t n_tracks,
                           const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba7_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (n_cams > 0 && !intrinsics) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = ba_check_tracks(n_cams, 3, n_tracks, track_ptr, obs_cam, obs_xy, "gsfm_ba7_problem_create")) return (gsfm_status)st;
  const size_t N = n_cams, T = n_tracks;
  hvec<uint32_t> order(n_tracks);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1), cmask(2 * N + T, 0);
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<gsfm_ba7_problem, void (*)(gsfm_ba7_problem*)> P(new gsfm_ba7_problem, gsfm_ba7_problem_destroy);
  ba_init(P.get(), n_cams, 3, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated, order.data());
  for (size_t k = 0; k < N; ++k) {
    if (focal_free && !focal_free[k]) P->h_active[2 * N + k] = 0;
    cmask[k] = P->h_active[N + k];
  }
  std::copy(P->h_active.begin() + 3 * N, P->h_active.end(), cmask.begin() + 2 * N);
  size_t zeroed = 0;
  if (int st = ba_commit_upload(P.get(), b7_place, "the focal-length bundle adjustment problem", track_ptr, order.data(), obs_cam, obs_xy, &zeroed)) return (gsfm_status)st;
  const hipStream_t s = P->mem.s;
  HIPCHK_S(ba_up(s, P->intrinsics, intrinsics, 24 * N)); HIPCHK_S(ba_up(s, P->cam_est, est.data(), N)); HIPCHK_S(ba_up(s, P->centroid_mask, cmask.data(), cmask.size()));
  if (int st = sync_stream(s, "focal-length bundle adjustment problem create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

gsfm_status b7_solve_impl(gsfm_ba7_problem* P, double* rot_aa, double* cam_pos, double* focal, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  if (int st = b7_check_point(P, rot_aa, cam_pos, focal, points)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks;
  hvec<double> stage;
  return ba_solve(P, b7_options(opt), summary, "ba7", [&] { return b7_upload_point(P, rot_aa, cam_pos, focal, points, &stage); }, [&](const double* xh) {
    for (size_t k = 0; k < N; ++k) {
      if (P->h_active[k]) { std::copy(&xh[3 * k], &xh[3 * k] + 3, rot_aa + 3 * k); std::copy(&xh[3 * (N + k)], &xh[3 * (N + k)] + 3, cam_pos + 3 * k); }
      if (P->h_active[2 * N + k]) focal[k] = xh[3 * (2 * N + k)];
    }
    for (size_t t = 0; t < T; ++t) if (P->h_active[3 * N + t]) std::copy(&xh[3 * (3 * N + t)], &xh[3 * (3 * N + t)] + 3, points + 3 * t);
  });
}

// node-ordered camera vector (3 N x 3) -> per camera w, o, f (N x 7)
void b7_interleave(const double* nodes, size_t N, double* out) {
  for (size_t k = 0; k < N; ++k) {
    for (int c = 0; c < 3; ++c) { out[7 * k + c] = nodes[3 * k + c]; out[7 * k + 3 + c] = nodes[3 * (N + k) + c]; }
    out[7 * k + 6] = nodes[3 * (2 * N + k)];
  }
}
// a node-ordered array's intrinsics nodes -> one double per camera
void b7_focal_column(const double* nodes, size_t N, double* out) { for (size_t k = 0; k < N; ++k) out[k] = nodes[3 * (2 * N + k)]; }

gsfm_status b7_linearize_impl(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* cost,
                              double* grad_rot, double* grad_pos, double* grad_focal, double* grad_point, double* diag_cam, double* diag_point) {
  if (int st = b7_check_point(P, rot_aa, cam_pos, focal, points)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = P->n_nodes;
  double c = 0.0;
  hvec<double> stage;
  if (int st = b7_upload_point(P, rot_aa, cam_pos, focal, points, &stage)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, b7_options(nullptr), &c)) return (gsfm_status)st;
  hvec<double> g3(3 * NN), d6(6 * NN), bx(GSFM_BA7_BX * N);
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g, 24 * NN, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg, 48 * NN, hipMemcpyDeviceToHost, P->mem.s));
  if (N) HIPCHK_S(hipMemcpyAsync(bx.data(), P->Bx, 8 * GSFM_BA7_BX * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearize outputs")) return (gsfm_status)st;
  if (grad_rot) std::copy(g3.begin(), g3.begin() + 3 * N, grad_rot);
  if (grad_pos) std::copy(g3.begin() + 3 * N, g3.begin() + 6 * N, grad_pos);
  if (grad_focal) b7_focal_column(g3.data(), N, grad_focal);
  if (grad_point) std::copy(g3.begin() + 9 * N, g3.end(), grad_point);
  auto sym = [&](size_t node, int r, int cc) {
    static const int idx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    return d6[6 * node + idx[r][cc]];
  };
  if (diag_cam)
    for (size_t k = 0; k < N; ++k) {
      double* B = diag_cam + 49 * k;
      const double* X = &bx[GSFM_BA7_BX * k];
      for (int r = 0; r < 3; ++r) {
        for (int cc = 0; cc < 3; ++cc) {
          B[7 * r + cc] = sym(k, r, cc); B[7 * (3 + r) + 3 + cc] = sym(N + k, r, cc);
          B[7 * r + 3 + cc] = X[3 * r + cc]; B[7 * (3 + cc) + r] = X[3 * r + cc];
        }
        B[7 * r + 6] = B[7 * 6 + r] = X[9 + r]; B[7 * (3 + r) + 6] = B[7 * 6 + 3 + r] = X[12 + r];
      }
      B[48] = d6[6 * (2 * N + k)];
    }
  if (diag_point)
    for (size_t t = 0; t < T; ++t)
      for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) diag_point[9 * t + 3 * r + cc] = sym(3 * N + t, r, cc);
  if (cost) *cost = c;
  return GSFM_OK;
}

gsfm_status b7_residuals_impl(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* r_out, double* rho_out) {
  if (!P || b7_needs_points(P, rot_aa, cam_pos, focal, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  hvec<double> stage;
  return ba_residuals(P, [&] { return b7_upload_point(P, rot_aa, cam_pos, focal, points, &stage); }, r_out, rho_out);
}

gsfm_status b7_schur_matvec_impl(gsfm_ba7_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b7_options(opt);
  const size_t N = P->n_cams;
  if (N == 0) return GSFM_OK;
  hvec<double> nodes(9 * N, 0.0), outn(9 * N);
  for (size_t k = 0; k < N; ++k) {
    for (int c = 0; c < 3; ++c) { nodes[3 * k + c] = v[7 * k + c]; nodes[3 * (N + k) + c] = v[7 * k + 3 + c]; }
    nodes[3 * (2 * N + k)] = v[7 * k + 6];
  }
  ba_jacobi_scale(P, o);
  b7_prep(P, radius, o);
  HIPCHK_S(hipMemcpyAsync(P->p, nodes.data(), 72 * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_ba_scale, ba_grid(3 * N), dim3(256), 0, P->mem.s, 3 * N, P->active, P->S, P->p, 1.0, P->q);
  b7_schur_product(P, P->q, P->p, P->Ap);
  HIPCHK_S(hipMemcpyAsync(outn.data(), P->Ap, 72 * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "schur_matvec")) return (gsfm_status)st;
  b7_interleave(outn.data(), N, y);
  return GSFM_OK;
}

gsfm_status b7_step_check_impl(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                               const gsfm_ba_options* opt, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out,
                               double* delta_focal_out, double* delta_point_out, double* jdelta_out, double* scal_out, int32_t* info_out) {
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b7_options(opt);
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs;
  DevBuf<char> scratch;
  if (jdelta_out && O > 0 && scratch.alloc(16 * O) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc J delta buffer");
  double* jd_dev = (jdelta_out && O > 0) ? (double*)scratch.p : nullptr;
  double cost = 0.0;
  hvec<double> stage;
  if (int st = b7_upload_point(P, rot_aa, cam_pos, focal, points, &stage)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
  BaStep step;
  if (int st = b7_step(P, radius, o, &step, jd_dev)) return (gsfm_status)st;
  double hs[BS_N];
  hvec<double> rhs_n(9 * N), yc_n(9 * N), df_n(3 * N);
  auto down = [&](double* dst, const double* src, size_t rows) { return (dst && rows) ? hipMemcpyAsync(dst, src, 24 * rows, hipMemcpyDeviceToHost, P->mem.s) : hipSuccess; };
  HIPCHK_S(hipMemcpyAsync(hs, P->scal, sizeof(hs), hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(down(rhs_n.data(), P->rhs, 3 * N)); HIPCHK_S(down(yc_n.data(), P->y, 3 * N)); HIPCHK_S(down(yp_out, P->y + 9 * N, T));
  HIPCHK_S(down(delta_rot_out, P->delta, N)); HIPCHK_S(down(delta_pos_out, P->delta + 3 * N, N)); HIPCHK_S(down(df_n.data(), P->delta + 6 * N, N));
  HIPCHK_S(down(delta_point_out, P->delta + 9 * N, T));
  if (jd_dev) HIPCHK_S(hipMemcpyAsync(jdelta_out, jd_dev, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "step check")) return (gsfm_status)st;
  if (rhs_out) b7_interleave(rhs_n.data(), N, rhs_out);
  if (yc_out) b7_interleave(yc_n.data(), N, yc_out);
  if (delta_focal_out) for (size_t k = 0; k < N; ++k) delta_focal_out[k] = df_n[3 * k];
  if (scal_out) {
    scal_out[0] = -hs[BS_DG] - 0.5 * hs[B6_JD2];   // the solve's model cost change
    scal_out[1] = hs[BS_DG]; scal_out[2] = hs[B6_JD2]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.cg; info_out[1] = step.stalled ? 1 : 0; }
  return GSFM_OK;
}

gsfm_status b7_time_kernels_impl(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                 int32_t reps, double* out_us) {
  DeviceGuard g(P->device);
  gsfm_ba_options o = b7_options(nullptr);
  double cost = 0.0;
  hvec<double> stage;
  if (int st = b7_upload_point(P, rot_aa, cam_pos, focal, points, &stage)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = b7_step(P, radius, o, &step)) return (gsfm_status)st;
  b7_cameras(P, P->x);
  KernelTimer timed{P->mem.s, reps, out_us};
  if (int st = timed.create()) return (gsfm_status)st;
  const uint32_t N = P->n_cams;
  timed([&] { b7_cameras(P, P->x); });
  timed([&] { B7_TRACKS(P, k_ba7_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_ba7_cam_lin, ba_row_grid(N), dim3(256), 0, P->mem.s, b7_dev(P), P->g, P->Dg, P->Bx); });
  timed([&] { B7_TRACKS(P, k_ba7_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { B7_TRACKS(P, k_ba7_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba7_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b7_dev(P), (const double*)P->q, (const double*)P->zt, 1.0, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba7_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b7_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv); });
  timed([&] { B7_TRACKS(P, k_ba7_quad_tracks, (const double*)P->delta, P->pt_scratch, (double*)nullptr); });
  return (gsfm_status)timed.st;
}

}  // namespace

void gsfm_ba7_problem::cost(const double* at, double* r_out, double* rho_out) { b7_cost(this, at, r_out, rho_out); }
void gsfm_ba7_problem::linearize() { b7_linearize(this); }
int gsfm_ba7_problem::step(double radius, const gsfm_ba_options& o, BaStep* out) { return b7_step(this, radius, o, out); }

extern "C" {

int gsfm_ba7_abi_version(void) { return GSFM_BA7_ABI_VERSION; }

// gsfm_ba6.h's defaults with a stall rule that looks further: see the header
void gsfm_ba7_options_default(gsfm_ba_options* o) {
  gsfm_ba6_options_default(o);
  o->cg_stall_iterations = o->max_cg_iterations / 2;
}

void gsfm_ba7_problem_destroy(gsfm_ba7_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

gsfm_status gsfm_ba7_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, const uint8_t* focal_free, uint64_t n_tracks,
                                    const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                    gsfm_ba7_problem** out) {
  return guarded("focal-length bundle adjustment problem creation", b7_create_impl, n_cams, intrinsics, cam_estimated, focal_free, n_tracks, track_ptr, obs_cam,
                 obs_xy, point_estimated, out);
}

gsfm_status gsfm_ba7_set_loss(gsfm_ba7_problem* P, const gsfm_loss_node* prog, int32_t n) { return ba_set_loss(P, prog, n, "focal-length bundle adjustment"); }

gsfm_status gsfm_ba7_solve(gsfm_ba7_problem* P, double* rot_aa, double* cam_pos, double* focal, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  return guarded("the focal-length bundle adjustment", b7_solve_impl, P, rot_aa, cam_pos, focal, points, opt, summary);
}

gsfm_status gsfm_ba7_residuals(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* r_out,
                               double* rho_out) {
  return guarded("focal-length bundle adjustment residuals", b7_residuals_impl, P, rot_aa, cam_pos, focal, points, r_out, rho_out);
}

gsfm_status gsfm_ba7_linearize(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* cost,
                               double* grad_rot, double* grad_pos, double* grad_focal, double* grad_point, double* diag_cam, double* diag_point) {
  return guarded("focal-length bundle adjustment linearisation", b7_linearize_impl, P, rot_aa, cam_pos, focal, points, cost, grad_rot, grad_pos, grad_focal,
                 grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_ba7_schur_matvec(gsfm_ba7_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_ba7_linearize or gsfm_ba7_step_check first");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("focal-length bundle adjustment Schur product", b7_schur_matvec_impl, P, v, radius, opt, y);
}

gsfm_status gsfm_ba7_step_check(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                const gsfm_ba_options* opt, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out,
                                double* delta_focal_out, double* delta_point_out, double* jdelta_out, double* scal_out, int32_t* info_out) {
  if (int st = b7_check_point(P, rot_aa, cam_pos, focal, points)) return (gsfm_status)st;
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("focal-length bundle adjustment step check", b7_step_check_impl, P, rot_aa, cam_pos, focal, points, radius, opt, rhs_out, yc_out, yp_out,
                 delta_rot_out, delta_pos_out, delta_focal_out, delta_point_out, jdelta_out, scal_out, info_out);
}

gsfm_status gsfm_ba7_time_kernels(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                  int32_t reps, double* out_us) {
  if (!P || !out_us) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = b7_check_point(P, rot_aa, cam_pos, focal, points)) return (gsfm_status)st;
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  return guarded("focal-length bundle adjustment kernel timing", b7_time_kernels_impl, P, rot_aa, cam_pos, focal, points, radius, reps, out_us);
}

}  // extern "C"
