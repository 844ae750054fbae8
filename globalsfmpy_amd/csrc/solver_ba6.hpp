// Host side of the full bundle adjustment (include/gsfm_ba6.h): orientations, positions and points.  The problem's common part, the
// Levenberg-Marquardt operations, the checks, solve, residuals and timing are solver_ba.hpp's; here are the kernels' launches
// (ba6_kernels.hpp), the Schur-complement PCG over the cameras' 2 N nodes (on lm_loop.hpp's driver, with the recurrence and the vector kernels
// of pos_kernels.hpp), and the step with its seven-direction gauge projection, whose 7 x 7 Gram system is solved here.
// The unknowns are one array of (2 n_cams + n_tracks) x 3: angle-axis vectors, centres, points.
#pragma once
#include "solver_ba.hpp"
#include "ba6_kernels.hpp"
#include "../../include/gsfm_ba6.h"

struct gsfm_ba6_problem : BaProblem {
  uint8_t* cam_est = nullptr;
  double *intrinsics = nullptr, *Jt = nullptr, *Rt = nullptr, *Jc = nullptr, *Bx = nullptr, *gpart = nullptr;
  void cost(const double* at, double* r_out, double* rho_out) override;
  void linearize() override;
  int step(double radius, const gsfm_ba_options& o, BaStep* out) override;
};

namespace {

using gsfm::Ba6Dev;

// the device scalars behind solver_ba.hpp's: the delta^T (J^T J) delta of the step is |J delta|^2 here
enum { B6_JD2 = BS_DLD, B6_COEF = BS_N /* 7 */, B6_GRAM = B6_COEF + GSFM_BA6_GAUGE /* 35 */, B6_N = B6_GRAM + GSFM_BA6_GDOTS };

Ba6Dev b6_dev(const gsfm_ba6_problem* P) {
  Ba6Dev a{};
  a.b = ba_dev_shared(P);
  a.Jt = P->Jt; a.Rt = P->Rt; a.Jc = P->Jc;
  return a;
}
#define B6_TRACKS(P, K, ...) ba_tracks(P, b6_dev(P), K<4>, K<16>, K<64>, __VA_ARGS__)

// the camera records (R, J_l) of the point `at`
void b6_cameras(gsfm_ba6_problem* P, const double* at) {
  if (P->n_cams) hipLaunchKernelGGL(k_ba6_cameras, ba_grid(P->n_cams), dim3(256), 0, P->mem.s, P->n_cams, at, (const double*)P->intrinsics, (const uint8_t*)P->cam_est, P->cams);
}
// cost of the point `at` into scal[BS_COST]
void b6_cost(gsfm_ba6_problem* P, const double* at, double* r_out = nullptr, double* rho_out = nullptr) {
  b6_cameras(P, at);
  B6_TRACKS(P, k_ba6_cost_tracks, at, P->pt_scratch, r_out, rho_out);
  ba_sum(P, P->pt_scratch, P->n_tracks, BS_COST);
}
void b6_linearize(gsfm_ba6_problem* P) {
  b6_cameras(P, P->x);
  B6_TRACKS(P, k_ba6_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(k_ba6_cam_lin, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, b6_dev(P), P->g, P->Dg, P->Bx);
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

// PCG on Sc y_c = rhs from y_c = 0 (k_ba6_pcg_init set r, z, p, q) over the cameras' 2 N nodes: lm_loop.hpp's driver, with the breakdown rule
int b6_pcg(gsfm_ba6_problem* P, const gsfm_ba_options& o, BaStep* out) {
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams, N2 = 2 * N;
  V.dot(P->r, P->z, nullptr, N2, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    b6_schur_product(P, P->q, P->p, P->Ap);
    V.dot(P->p, P->Ap, nullptr, N2, BS_PAP);
    hipLaunchKernelGGL(k_ba6_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, N2, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N2), dim3(256), 0, P->mem.s, N2, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, true, iterate, V.pcg_reader(), &out->cg, &out->stalled, &out->cg_rel);
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
// gsfm_ba6_step_check.  Leaves y, delta, the trial point P->cand and scal[BS_STEP2], [BS_DG], [B6_JD2] enqueued.  jd_out: device, may be NULL.
int b6_step(gsfm_ba6_problem* P, double radius, const gsfm_ba_options& o, BaStep* out, double* jd_out = nullptr) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes;
  const DevScalars V = P->vec();
  *out = BaStep();
  b6_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_ba6_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)nullptr, (const double*)P->zt, -1.0, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_ba6_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv);
  hipLaunchKernelGGL(k_ba6_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = b6_pcg(P, o, out)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(2 * (size_t)N), dim3(256), 0, P->mem.s, 2 * (size_t)N, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) B6_TRACKS(P, k_ba6_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->b, -1.0, P->y + 6 * (size_t)N, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  const bool project = o.remove_gauge && P->n_active > 0;
  const double inv_count = P->n_active > 0 ? 1.0 / (double)P->n_active : 0.0;
  if (project) {
    for (int c = 0; c < 3; ++c) {
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)(P->x + 3 * (size_t)N), P->active + N, (size_t)N + T, c, P->part);
      V.reduce(BS_SUMX + c);
    }
    hipLaunchKernelGGL(k_ba6_gauge_dots, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->delta,
                       (const double*)P->scal, (int)BS_SUMX, inv_count, P->gpart);
    hipLaunchKernelGGL(k_ba6_gauge_reduce, dim3(GSFM_BA6_GDOTS), dim3(256), 0, P->mem.s, (const double*)P->gpart, P->scal + B6_GRAM);
    double dots[GSFM_BA6_GDOTS], coef[GSFM_BA6_GAUGE];
    if (int st = V.read(dots, P->scal + B6_GRAM, sizeof(dots), "gauge dots")) return st;
    b6_gauge_solve(dots, coef);
    HIPCHK(hipMemcpyAsync(P->scal + B6_COEF, coef, sizeof(coef), hipMemcpyHostToDevice, P->mem.s));
    if (int st = sync_stream(P->mem.s, "gauge coefficients")) return st;   // (coef is a local)
  }
  hipLaunchKernelGGL(k_ba6_gauge_apply, ba_grid(NN), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->scal, (int)BS_SUMX, inv_count,
                     (int)B6_COEF, project ? 1 : 0, P->delta, P->cand);
  V.dot(P->delta, P->delta, nullptr, NN, BS_STEP2);
  V.dot(P->delta, P->g, nullptr, NN, BS_DG);
  B6_TRACKS(P, k_ba6_quad_tracks, (const double*)P->delta, P->pt_scratch, jd_out);
  ba_sum(P, P->pt_scratch, T, B6_JD2);
  return 0;
}

gsfm_ba_options b6_options(const gsfm_ba_options* opt) { return ba_options(opt, gsfm_ba6_options_default); }

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
  return ba_setup_linearize(P, o, cost);
}
bool b6_needs_points(const gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points) {
  return (P->n_cams > 0 && (!rot_aa || !cam_pos)) || (P->n_tracks > 0 && !points);
}

FlatLayout b6_place(gsfm_ba6_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  SlabTake take{FlatLayout(), slab};
  take(P->scal, B6_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 6 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Bx, 9 * N);
  *zeroed = take.L.total;
  take(P->Minv, 36 * N); take(P->Cinv, 18 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS); take(P->gpart, (size_t)GSFM_BA6_GDOTS * GSFM_POS_PARTS);
  take(P->cams, GSFM_BA6_CAM_DOUBLES * N); take(P->intrinsics, 3 * N); take(P->Jt, 12 * O); take(P->Rt, 2 * O); take(P->Jc, 12 * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN); take(P->cam_est, N);
  return take.L;
}

gsfm_status b6_create_impl(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                           const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba6_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (n_cams > 0 && !intrinsics) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = ba_check_tracks(n_cams, 2, n_tracks, track_ptr, obs_cam, obs_xy, "gsfm_ba6_problem_create")) return (gsfm_status)st;
  const size_t N = n_cams;
  hvec<uint32_t> order(n_tracks);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1);
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<gsfm_ba6_problem, void (*)(gsfm_ba6_problem*)> P(new gsfm_ba6_problem, gsfm_ba6_problem_destroy);
  ba_init(P.get(), n_cams, 2, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated, order.data());
  size_t zeroed = 0;
  if (int st = ba_commit_upload(P.get(), b6_place, "the full bundle adjustment problem", track_ptr, order.data(), obs_cam, obs_xy, &zeroed)) return (gsfm_status)st;
  const hipStream_t s = P->mem.s;
  HIPCHK_S(ba_up(s, P->intrinsics, intrinsics, 24 * N)); HIPCHK_S(ba_up(s, P->cam_est, est.data(), N));
  if (int st = sync_stream(s, "full bundle adjustment problem create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

gsfm_status b6_solve_impl(gsfm_ba6_problem* P, double* rot_aa, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  if (!P || b6_needs_points(P, rot_aa, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks;
  return ba_solve(P, b6_options(opt), summary, "ba6", [&] { return b6_upload_point(P, rot_aa, cam_pos, points); }, [&](const double* xh) {
    for (size_t k = 0; k < N; ++k)
      if (P->h_active[k]) { std::copy(&xh[3 * k], &xh[3 * k] + 3, rot_aa + 3 * k); std::copy(&xh[3 * (N + k)], &xh[3 * (N + k)] + 3, cam_pos + 3 * k); }
    for (size_t t = 0; t < T; ++t) if (P->h_active[2 * N + t]) std::copy(&xh[3 * (2 * N + t)], &xh[3 * (2 * N + t)] + 3, points + 3 * t);
  });
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
  double c = 0.0;
  if (int st = b6_setup_linearize(P, rot_aa, cam_pos, points, b6_options(nullptr), &c)) return (gsfm_status)st;
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
  return ba_residuals(P, [&] { return b6_upload_point(P, rot_aa, cam_pos, points); }, r_out, rho_out);
}

gsfm_status b6_schur_matvec_impl(gsfm_ba6_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  DeviceGuard g(P->device);
  const gsfm_ba_options o = b6_options(opt);
  const size_t N = P->n_cams;
  if (N == 0) return GSFM_OK;
  hvec<double> nodes(6 * N), outn(6 * N);
  for (size_t k = 0; k < N; ++k) for (int c = 0; c < 3; ++c) { nodes[3 * k + c] = v[6 * k + c]; nodes[3 * (N + k) + c] = v[6 * k + 3 + c]; }
  ba_jacobi_scale(P, o);
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
  double hs[BS_N];
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
    scal_out[0] = -hs[BS_DG] - 0.5 * hs[B6_JD2];   // the solve's model cost change
    scal_out[1] = hs[BS_DG]; scal_out[2] = hs[B6_JD2]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.cg; info_out[1] = step.stalled ? 1 : 0; }
  return GSFM_OK;
}

gsfm_status b6_time_kernels_impl(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us) {
  DeviceGuard g(P->device);
  gsfm_ba_options o = b6_options(nullptr);
  double cost = 0.0;
  if (int st = b6_setup_linearize(P, rot_aa, cam_pos, points, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = b6_step(P, radius, o, &step)) return (gsfm_status)st;
  b6_cameras(P, P->x);       // (the step's trial cost is not evaluated here; the records are those of x)
  KernelTimer timed{P->mem.s, reps, out_us};
  if (int st = timed.create()) return (gsfm_status)st;
  const uint32_t N = P->n_cams;
  timed([&] { b6_cameras(P, P->x); });
  timed([&] { B6_TRACKS(P, k_ba6_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_lin, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), P->g, P->Dg, P->Bx); });
  timed([&] { B6_TRACKS(P, k_ba6_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { B6_TRACKS(P, k_ba6_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->q, (const double*)P->zt, 1.0, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba6_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, b6_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv); });
  timed([&] { B6_TRACKS(P, k_ba6_quad_tracks, (const double*)P->delta, P->pt_scratch, (double*)nullptr); });
  return (gsfm_status)timed.st;
}

}  // namespace

void gsfm_ba6_problem::cost(const double* at, double* r_out, double* rho_out) { b6_cost(this, at, r_out, rho_out); }
void gsfm_ba6_problem::linearize() { b6_linearize(this); }
int gsfm_ba6_problem::step(double radius, const gsfm_ba_options& o, BaStep* out) { return b6_step(this, radius, o, out); }

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

gsfm_status gsfm_ba6_set_loss(gsfm_ba6_problem* P, const gsfm_loss_node* prog, int32_t n) { return ba_set_loss(P, prog, n, "full bundle adjustment"); }

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
