// Host side of the full bundle adjustment in both of its forms: orientations, positions and points (include/gsfm_ba6.h, camera dimension
// D = 6) and the same with free focal lengths (include/gsfm_ba7.h, D = 7).  One implementation, templated on the problem type, from which the
// two C ABIs are instantiated.  The problem's common part, the Levenberg-Marquardt operations, the checks, solve, residuals and timing are
// solver_ba.hpp's; here are the kernels' launches (full_ba_kernels.hpp), the Schur-complement PCG over the cameras' nodes (on lm_loop.hpp's
// driver, with the recurrence and the vector kernels of pos_kernels.hpp), and the step with its seven-direction gauge projection, whose 7 x 7
// Gram system is solved here.
// The unknowns are one array of (NODES n_cams + n_tracks) x 3: angle-axis vectors, centres, at D = 7 intrinsics nodes (f, 0, 0), points.  A
// camera counts as NODES = 2 or 3 nodes; the intrinsics node's active byte is `camera active && focal_free` (full_ba_kernels.hpp states the
// invariant on its padding).  What differs between the two forms: the upload of the point (the staged intrinsics nodes), the focal test of
// fba_check_point, the centroid's mask, the N x D packing of camera vectors and the unpacking of diag_cam.
#pragma once
#include "solver_ba.hpp"
#include "full_ba_kernels.hpp"
#include "../../include/gsfm_ba6.h"
#include "../../include/gsfm_ba7.h"

#include <type_traits>

template <int D_> struct FullBaShared : BaProblem {
  static constexpr int D = D_;
  using Problem = std::conditional_t<D_ == 6, gsfm_ba6_problem, gsfm_ba7_problem>;
  uint8_t* cam_est = nullptr;
  double *intrinsics = nullptr, *Jt = nullptr, *Rt = nullptr, *Jc = nullptr, *Bx = nullptr, *gpart = nullptr;
  void cost(const double* at, double* r_out, double* rho_out) override;
  void linearize() override;
  int step(double radius, const gsfm_ba_options& o, BaStep* out) override;
};
// (the names: the entry in the no-device message, the slab's owner, the wait at the end of create, the verbose line's tag)
struct gsfm_ba6_problem : FullBaShared<6> {
  static constexpr const char *create_entry = "gsfm_ba6_problem_create", *slab_owner = "the full bundle adjustment problem",
                              *create_wait = "full bundle adjustment problem create", *tag = "ba6";
  static constexpr auto options_default = gsfm_ba6_options_default;
  const uint8_t* centroid() const { return active + n_cams; }   // the centres and points follow the orientations
};
struct gsfm_ba7_problem : FullBaShared<7> {
  static constexpr const char *create_entry = "gsfm_ba7_problem_create", *slab_owner = "the focal-length bundle adjustment problem",
                              *create_wait = "focal-length bundle adjustment problem create", *tag = "ba7";
  static constexpr auto options_default = gsfm_ba7_options_default;
  uint8_t* centroid_mask = nullptr;   // `active` from the centres on with zeros on the intrinsics nodes
  const uint8_t* centroid() const { return centroid_mask; }
};

namespace {

using gsfm::Fba;
using gsfm::FbaDev;
using gsfm::fba_at;

// the device scalars behind solver_ba.hpp's: the delta^T (J^T J) delta of the step is |J delta|^2 here
enum { FB_JD2 = BS_DLD, FB_COEF = BS_N /* 7 */, FB_GRAM = FB_COEF + GSFM_BA6_GAUGE /* 35 */, FB_N = FB_GRAM + GSFM_BA6_GDOTS };

// the caller's point: orientations, centres, focal lengths (D = 7; else NULL) and points
struct FbaPoint { const double *rot_aa, *cam_pos, *focal, *points; };

template <typename Pb> FbaDev fba_dev(const Pb* P) {
  FbaDev a{};
  a.b = ba_dev_shared(P);
  a.Jt = P->Jt; a.Rt = P->Rt; a.Jc = P->Jc;
  return a;
}
#define FBA_TRACKS(P, K, ...) ba_tracks(P, fba_dev(P), K<D, 4>, K<D, 16>, K<D, 64>, __VA_ARGS__)

// the camera records (R, J_l; D = 7: f) of the point `at`
template <typename Pb> void fba_cameras(Pb* P, const double* at) {
  if (P->n_cams) hipLaunchKernelGGL(k_fba_cameras<Pb::D>, ba_grid(P->n_cams), dim3(256), 0, P->mem.s, P->n_cams, at, (const double*)P->intrinsics, (const uint8_t*)P->cam_est, P->cams);
}
// cost of the point `at` into scal[BS_COST]
template <typename Pb> void fba_cost(Pb* P, const double* at, double* r_out = nullptr, double* rho_out = nullptr) {
  fba_cameras(P, at);
  ba_tracks(P, fba_dev(P), k_fba_cost_tracks<4>, k_fba_cost_tracks<16>, k_fba_cost_tracks<64>, (size_t)Fba<Pb::D>::NODES * P->n_cams, at, P->pt_scratch, r_out, rho_out);
  ba_sum(P, P->pt_scratch, P->n_tracks, BS_COST);
}
template <typename Pb> void fba_linearize(Pb* P) {
  constexpr int D = Pb::D;
  fba_cameras(P, P->x);
  FBA_TRACKS(P, k_fba_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(k_fba_cam_lin<D>, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, fba_dev(P), P->g, P->Dg, P->Bx);
}
template <typename Pb> void fba_prep(Pb* P, double radius, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_ba_prep_nodes, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, P->n_nodes, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal,
                     o.max_lm_diagonal, P->D2, P->b);
  // (the points are the nodes from NODES n_cams on; their inverses are refined: full_ba_kernels.hpp)
  hipLaunchKernelGGL(k_ba6_prep_points, ba_grid(P->n_tracks), dim3(256), 0, P->mem.s, Fba<Pb::D>::NODES * P->n_cams, P->n_tracks, P->active, P->Dg, P->S, P->D2, P->b,
                     P->Cinv, P->Gt, P->zt);
}
template <typename Pb> void fba_schur_product(Pb* P, const double* qvec, const double* pvec, double* out) {
  constexpr int D = Pb::D;
  FBA_TRACKS(P, k_fba_point_pass, qvec, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1);
  hipLaunchKernelGGL(k_fba_cam_pass<D>, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, fba_dev(P), qvec, (const double*)P->zt, 1.0, pvec, (const double*)P->S,
                     (const double*)P->D2, (const double*)nullptr, out, 1);
}

// PCG on Sc y_c = rhs from y_c = 0 (k_fba_pcg_init set r, z, p, q) over the cameras' NODES N nodes: lm_loop.hpp's driver, with the breakdown rule
template <typename Pb> int fba_pcg(Pb* P, const gsfm_ba_options& o, BaStep* out) {
  constexpr int D = Pb::D;
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams, NC = Fba<D>::NODES * N;
  V.dot(P->r, P->z, nullptr, NC, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    fba_schur_product(P, P->q, P->p, P->Ap);
    V.dot(P->p, P->Ap, nullptr, NC, BS_PAP);
    hipLaunchKernelGGL(k_fba_pcg_update<D>, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, NC, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(NC), dim3(256), 0, P->mem.s, NC, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, true, iterate, V.pcg_reader(), &out->cg, &out->stalled, &out->cg_rel);
}

// (V^T V) c = V^T delta by Cholesky without pivoting; a direction whose pivot is not above 1e-12 of its own squared norm keeps c = 0
void fba_gauge_solve(const double* dots, double* c) {
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
// gsfm_ba*_step_check.  Leaves y, delta, the trial point P->cand and scal[BS_STEP2], [BS_DG], [FB_JD2] enqueued.  jd_out: device, may be NULL.
template <typename Pb> int fba_step(Pb* P, double radius, const gsfm_ba_options& o, BaStep* out, double* jd_out = nullptr) {
  constexpr int D = Pb::D;
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes, NC = Fba<D>::NODES * (size_t)N;
  const DevScalars V = P->vec();
  *out = BaStep();
  fba_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_fba_cam_pass<D>, ba_row_grid(N), dim3(256), 0, P->mem.s, fba_dev(P), (const double*)nullptr, (const double*)P->zt, -1.0, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_fba_cam_precond<D>, ba_row_grid(N), dim3(256), 0, P->mem.s, fba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv);
  hipLaunchKernelGGL(k_fba_pcg_init<D>, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = fba_pcg(P, o, out)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NC), dim3(256), 0, P->mem.s, NC, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) FBA_TRACKS(P, k_fba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->b, -1.0, P->y + 3 * NC, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  const bool project = o.remove_gauge && P->n_active > 0;
  const double inv_count = P->n_active > 0 ? 1.0 / (double)P->n_active : 0.0;
  if (project) {
    for (int c = 0; c < 3; ++c) {   // the centroid of the active centres and points (D = 7: the intrinsics nodes between them are masked out)
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)(P->x + 3 * (size_t)N), P->centroid(), NN - N, c, P->part);
      V.reduce(BS_SUMX + c);
    }
    hipLaunchKernelGGL(D == 6 ? k_ba6_gauge_dots : k_ba7_gauge_dots, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->delta,
                       (const double*)P->scal, (int)BS_SUMX, inv_count, P->gpart);
    hipLaunchKernelGGL(k_ba6_gauge_reduce, dim3(GSFM_BA6_GDOTS), dim3(256), 0, P->mem.s, (const double*)P->gpart, P->scal + FB_GRAM);
    double dots[GSFM_BA6_GDOTS], coef[GSFM_BA6_GAUGE];
    if (int st = V.read(dots, P->scal + FB_GRAM, sizeof(dots), "gauge dots")) return st;
    fba_gauge_solve(dots, coef);
    HIPCHK(hipMemcpyAsync(P->scal + FB_COEF, coef, sizeof(coef), hipMemcpyHostToDevice, P->mem.s));
    if (int st = sync_stream(P->mem.s, "gauge coefficients")) return st;   // (coef is a local)
  }
  hipLaunchKernelGGL(D == 6 ? k_ba6_gauge_apply : k_ba7_gauge_apply, ba_grid(NN), dim3(256), 0, P->mem.s, N, NN, P->active, (const double*)P->x, (const double*)P->scal, (int)BS_SUMX, inv_count,
                     (int)FB_COEF, project ? 1 : 0, P->delta, P->cand);
  V.dot(P->delta, P->delta, nullptr, NN, BS_STEP2);
  V.dot(P->delta, P->g, nullptr, NN, BS_DG);
  FBA_TRACKS(P, k_fba_quad_tracks, (const double*)P->delta, P->pt_scratch, jd_out);
  ba_sum(P, P->pt_scratch, T, FB_JD2);
  return 0;
}

template <typename Pb> gsfm_ba_options fba_options(const gsfm_ba_options* opt) { return ba_options(opt, Pb::options_default); }

template <typename Pb> bool fba_needs_points(const Pb* P, const FbaPoint& at) {
  return (P->n_cams > 0 && (!at.rot_aa || !at.cam_pos || (Pb::D == 7 && !at.focal))) || (P->n_tracks > 0 && !at.points);
}
// NULL arguments and, at D = 7, the focal lengths of the active cameras, before any device call
template <typename Pb> int fba_check_point(const Pb* P, const FbaPoint& at) {
  if (!P || fba_needs_points(P, at)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if constexpr (Pb::D == 7)
    for (size_t k = 0; k < P->n_cams; ++k)
      if (P->h_active[k] && !(std::isfinite(at.focal[k]) && at.focal[k] > 0.0)) return fail(GSFM_ERR_INVALID_ARG, "the focal length of an active camera must be finite and positive");
  return 0;
}

// x = (rot_aa, cam_pos, [(f, 0, 0),] points), enqueued; stage must outlive the stream's copy of it (the callers wait before they return)
template <typename Pb> int fba_upload_point(Pb* P, const FbaPoint& at, hvec<double>* stage) {
  const size_t N = P->n_cams;
  if (N) {
    HIPCHK(hipMemcpyAsync(P->x, at.rot_aa, 24 * N, hipMemcpyHostToDevice, P->mem.s));
    HIPCHK(hipMemcpyAsync(P->x + 3 * N, at.cam_pos, 24 * N, hipMemcpyHostToDevice, P->mem.s));
    if constexpr (Pb::D == 7) {
      stage->assign(3 * N, 0.0);
      for (size_t k = 0; k < N; ++k) (*stage)[3 * k] = at.focal[k];
      HIPCHK(hipMemcpyAsync(P->x + 6 * N, stage->data(), 24 * N, hipMemcpyHostToDevice, P->mem.s));
    }
  }
  if (P->n_tracks) HIPCHK(hipMemcpyAsync(P->x + 3 * Fba<Pb::D>::NODES * N, at.points, 24 * (size_t)P->n_tracks, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}
template <typename Pb> int fba_setup_linearize(Pb* P, const FbaPoint& at, hvec<double>* stage, const gsfm_ba_options& o, double* cost) {
  if (int st = fba_upload_point(P, at, stage)) return st;
  return ba_setup_linearize(P, o, cost);
}

template <typename Pb> FlatLayout fba_place(Pb* P, char* slab, size_t* zeroed) {
  constexpr int D = Pb::D, NODES = Fba<D>::NODES;
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  SlabTake take{FlatLayout(), slab};
  take(P->scal, FB_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 3 * NODES * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Bx, Fba<D>::BX * N);
  *zeroed = take.L.total;
  take(P->Minv, D * D * N); take(P->Cinv, 18 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS); take(P->gpart, (size_t)GSFM_BA6_GDOTS * GSFM_POS_PARTS);
  take(P->cams, GSFM_BA6_CAM_DOUBLES * N); take(P->intrinsics, 3 * N); take(P->Jt, Fba<D>::J * O); take(P->Rt, 2 * O); take(P->Jc, Fba<D>::J * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN); take(P->cam_est, N);
  if constexpr (D == 7) take(P->centroid_mask, 2 * N + T);
  return take.L;
}

template <typename Pb> void fba_destroy(Pb* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

// focal_free: D = 7 (NULL: every focal length is free)
template <typename Pb>
gsfm_status fba_create_impl(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, const uint8_t* focal_free, uint64_t n_tracks,
                            const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, Pb** out) {
  constexpr int NODES = Fba<Pb::D>::NODES;
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (n_cams > 0 && !intrinsics) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = ba_check_tracks(n_cams, NODES, n_tracks, track_ptr, obs_cam, obs_xy, Pb::create_entry)) return (gsfm_status)st;
  const size_t N = n_cams, T = n_tracks;
  hvec<uint32_t> order(n_tracks);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1), cmask;
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<Pb, void (*)(Pb*)> P(new Pb, fba_destroy<Pb>);
  ba_init(P.get(), n_cams, NODES, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated, order.data());
  if constexpr (Pb::D == 7) {
    cmask.assign(2 * N + T, 0);
    for (size_t k = 0; k < N; ++k) {
      if (focal_free && !focal_free[k]) P->h_active[2 * N + k] = 0;
      cmask[k] = P->h_active[N + k];
    }
    std::copy(P->h_active.begin() + 3 * N, P->h_active.end(), cmask.begin() + 2 * N);
  }
  size_t zeroed = 0;
  if (int st = ba_commit_upload(P.get(), fba_place<Pb>, Pb::slab_owner, track_ptr, order.data(), obs_cam, obs_xy, &zeroed)) return (gsfm_status)st;
  const hipStream_t s = P->mem.s;
  HIPCHK_S(ba_up(s, P->intrinsics, intrinsics, 24 * N)); HIPCHK_S(ba_up(s, P->cam_est, est.data(), N));
  if constexpr (Pb::D == 7) { HIPCHK_S(ba_up(s, P->centroid_mask, cmask.data(), cmask.size())); }
  if (int st = sync_stream(s, Pb::create_wait)) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

// focal: D = 7
template <typename Pb>
gsfm_status fba_solve_impl(Pb* P, double* rot_aa, double* cam_pos, double* focal, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  constexpr int NODES = Fba<Pb::D>::NODES;
  const FbaPoint at{rot_aa, cam_pos, focal, points};
  if (int st = fba_check_point(P, at)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks;
  hvec<double> stage;
  return ba_solve(P, fba_options<Pb>(opt), summary, Pb::tag, [&] { return fba_upload_point(P, at, &stage); }, [&](const double* xh) {
    for (size_t k = 0; k < N; ++k) {
      if (P->h_active[k]) { std::copy(&xh[3 * k], &xh[3 * k] + 3, rot_aa + 3 * k); std::copy(&xh[3 * (N + k)], &xh[3 * (N + k)] + 3, cam_pos + 3 * k); }
      if constexpr (Pb::D == 7) if (P->h_active[2 * N + k]) focal[k] = xh[3 * (2 * N + k)];
    }
    for (size_t t = 0; t < T; ++t) if (P->h_active[NODES * N + t]) std::copy(&xh[3 * (NODES * N + t)], &xh[3 * (NODES * N + t)] + 3, points + 3 * t);
  });
}

// node-ordered camera vector (NODES N x 3) -> per camera w, o(, f) (N x D), and back
template <int D> void fba_pack(const double* nodes, size_t N, double* out) {
  for (size_t k = 0; k < N; ++k) for (int c = 0; c < D; ++c) out[D * k + c] = nodes[fba_at<D>(N, k, c)];
}
template <int D> void fba_unpack(const double* v, size_t N, double* nodes) {
  for (size_t k = 0; k < N; ++k) for (int c = 0; c < D; ++c) nodes[fba_at<D>(N, k, c)] = v[D * k + c];
}

// grad_focal: D = 7
template <typename Pb>
gsfm_status fba_linearize_impl(Pb* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* cost, double* grad_rot,
                               double* grad_pos, double* grad_focal, double* grad_point, double* diag_cam, double* diag_point) {
  constexpr int D = Pb::D, NODES = Fba<D>::NODES, BX = Fba<D>::BX;
  const FbaPoint at{rot_aa, cam_pos, focal, points};
  if (int st = fba_check_point(P, at)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = P->n_nodes;
  double c = 0.0;
  hvec<double> stage;
  if (int st = fba_setup_linearize(P, at, &stage, fba_options<Pb>(nullptr), &c)) return (gsfm_status)st;
  hvec<double> g3(3 * NN), d6(6 * NN), bx(BX * N);
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g, 24 * NN, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg, 48 * NN, hipMemcpyDeviceToHost, P->mem.s));
  if (N) HIPCHK_S(hipMemcpyAsync(bx.data(), P->Bx, 8 * BX * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearize outputs")) return (gsfm_status)st;
  if (grad_rot) std::copy(g3.begin(), g3.begin() + 3 * N, grad_rot);
  if (grad_pos) std::copy(g3.begin() + 3 * N, g3.begin() + 6 * N, grad_pos);
  if (D == 7 && grad_focal) for (size_t k = 0; k < N; ++k) grad_focal[k] = g3[3 * (2 * N + k)];
  if (grad_point) std::copy(g3.begin() + 3 * NODES * N, g3.end(), grad_point);
  auto sym = [&](size_t node, int r, int cc) {
    static const int idx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    return d6[6 * node + idx[r][cc]];
  };
  if (diag_cam)
    for (size_t k = 0; k < N; ++k) {
      double* B = diag_cam + D * D * k;
      const double* X = &bx[BX * k];
      for (int r = 0; r < 3; ++r) {
        for (int cc = 0; cc < 3; ++cc) {
          B[D * r + cc] = sym(k, r, cc); B[D * (3 + r) + 3 + cc] = sym(N + k, r, cc);
          B[D * r + 3 + cc] = X[3 * r + cc]; B[D * (3 + cc) + r] = X[3 * r + cc];
        }
        if constexpr (D == 7) { B[7 * r + 6] = B[7 * 6 + r] = X[9 + r]; B[7 * (3 + r) + 6] = B[7 * 6 + 3 + r] = X[12 + r]; }
      }
      if constexpr (D == 7) B[48] = d6[6 * (2 * N + k)];
    }
  if (diag_point)
    for (size_t t = 0; t < T; ++t)
      for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) diag_point[9 * t + 3 * r + cc] = sym(NODES * N + t, r, cc);
  if (cost) *cost = c;
  return GSFM_OK;
}

template <typename Pb>
gsfm_status fba_residuals_impl(Pb* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* r_out, double* rho_out) {
  const FbaPoint at{rot_aa, cam_pos, focal, points};
  if (!P || fba_needs_points(P, at)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  hvec<double> stage;
  return ba_residuals(P, [&] { return fba_upload_point(P, at, &stage); }, r_out, rho_out);
}

template <typename Pb> gsfm_status fba_schur_matvec_impl(Pb* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  constexpr int D = Pb::D, NODES = Fba<D>::NODES;
  DeviceGuard g(P->device);
  const gsfm_ba_options o = fba_options<Pb>(opt);
  const size_t N = P->n_cams;
  if (N == 0) return GSFM_OK;
  hvec<double> nodes(3 * NODES * N, 0.0), outn(3 * NODES * N);
  fba_unpack<D>(v, N, nodes.data());
  ba_jacobi_scale(P, o);
  fba_prep(P, radius, o);
  HIPCHK_S(hipMemcpyAsync(P->p, nodes.data(), 24 * NODES * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NODES * N), dim3(256), 0, P->mem.s, NODES * N, P->active, P->S, P->p, 1.0, P->q);
  fba_schur_product(P, P->q, P->p, P->Ap);
  HIPCHK_S(hipMemcpyAsync(outn.data(), P->Ap, 24 * NODES * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "schur_matvec")) return (gsfm_status)st;
  fba_pack<D>(outn.data(), N, y);
  return GSFM_OK;
}

// focal, delta_focal_out: D = 7
template <typename Pb>
gsfm_status fba_step_check_impl(Pb* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                const gsfm_ba_options* opt, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out,
                                double* delta_focal_out, double* delta_point_out, double* jdelta_out, double* scal_out, int32_t* info_out) {
  constexpr int D = Pb::D, NODES = Fba<D>::NODES;
  DeviceGuard g(P->device);
  const gsfm_ba_options o = fba_options<Pb>(opt);
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs;
  DevBuf<char> scratch;
  if (jdelta_out && O > 0 && scratch.alloc(16 * O) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc J delta buffer");
  double* jd_dev = (jdelta_out && O > 0) ? (double*)scratch.p : nullptr;
  double cost = 0.0;
  hvec<double> stage;
  if (int st = fba_setup_linearize(P, FbaPoint{rot_aa, cam_pos, focal, points}, &stage, o, &cost)) return (gsfm_status)st;
  BaStep step;
  if (int st = fba_step(P, radius, o, &step, jd_dev)) return (gsfm_status)st;
  double hs[BS_N];
  hvec<double> rhs_n(3 * NODES * N), yc_n(3 * NODES * N), df_n(D == 7 ? 3 * N : 0);
  auto down = [&](double* dst, const double* src, size_t rows) { return (dst && rows) ? hipMemcpyAsync(dst, src, 24 * rows, hipMemcpyDeviceToHost, P->mem.s) : hipSuccess; };
  HIPCHK_S(hipMemcpyAsync(hs, P->scal, sizeof(hs), hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(down(rhs_n.data(), P->rhs, NODES * N)); HIPCHK_S(down(yc_n.data(), P->y, NODES * N)); HIPCHK_S(down(yp_out, P->y + 3 * NODES * N, T));
  HIPCHK_S(down(delta_rot_out, P->delta, N)); HIPCHK_S(down(delta_pos_out, P->delta + 3 * N, N));
  if constexpr (D == 7) { HIPCHK_S(down(df_n.data(), P->delta + 6 * N, N)); }
  HIPCHK_S(down(delta_point_out, P->delta + 3 * NODES * N, T));
  if (jd_dev) HIPCHK_S(hipMemcpyAsync(jdelta_out, jd_dev, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "step check")) return (gsfm_status)st;
  if (rhs_out) fba_pack<D>(rhs_n.data(), N, rhs_out);
  if (yc_out) fba_pack<D>(yc_n.data(), N, yc_out);
  if (D == 7 && delta_focal_out) for (size_t k = 0; k < N; ++k) delta_focal_out[k] = df_n[3 * k];
  if (scal_out) {
    scal_out[0] = -hs[BS_DG] - 0.5 * hs[FB_JD2];   // the solve's model cost change
    scal_out[1] = hs[BS_DG]; scal_out[2] = hs[FB_JD2]; scal_out[3] = step.cg_rel;
  }
  if (info_out) { info_out[0] = step.cg; info_out[1] = step.stalled ? 1 : 0; }
  return GSFM_OK;
}

template <typename Pb>
gsfm_status fba_time_kernels_impl(Pb* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius, int32_t reps,
                                  double* out_us) {
  constexpr int D = Pb::D;
  DeviceGuard g(P->device);
  gsfm_ba_options o = fba_options<Pb>(nullptr);
  double cost = 0.0;
  hvec<double> stage;
  if (int st = fba_setup_linearize(P, FbaPoint{rot_aa, cam_pos, focal, points}, &stage, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = fba_step(P, radius, o, &step)) return (gsfm_status)st;
  fba_cameras(P, P->x);       // (the step's trial cost is not evaluated here; the records are those of x)
  KernelTimer timed{P->mem.s, reps, out_us};
  if (int st = timed.create()) return (gsfm_status)st;
  const uint32_t N = P->n_cams;
  timed([&] { fba_cameras(P, P->x); });
  timed([&] { FBA_TRACKS(P, k_fba_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_fba_cam_lin<D>, ba_row_grid(N), dim3(256), 0, P->mem.s, fba_dev(P), P->g, P->Dg, P->Bx); });
  timed([&] { ba_tracks(P, fba_dev(P), k_fba_cost_tracks<4>, k_fba_cost_tracks<16>, k_fba_cost_tracks<64>, (size_t)Fba<D>::NODES * N, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { FBA_TRACKS(P, k_fba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)nullptr, 1.0, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_fba_cam_pass<D>, ba_row_grid(N), dim3(256), 0, P->mem.s, fba_dev(P), (const double*)P->q, (const double*)P->zt, 1.0, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_fba_cam_precond<D>, ba_row_grid(N), dim3(256), 0, P->mem.s, fba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Dg, (const double*)P->Bx, P->Minv); });
  timed([&] { FBA_TRACKS(P, k_fba_quad_tracks, (const double*)P->delta, P->pt_scratch, (double*)nullptr); });
  return (gsfm_status)timed.st;
}

// what both C ABIs check before gsfm_ba*_schur_matvec and around a radius
template <typename Pb> int fba_check_matvec(const Pb* P, const double* v, double radius, const double* y, const char* call_first) {
  if (!P || !v || !y) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return fail(GSFM_ERR_INVALID_ARG, call_first);
  if (!(radius > 0.0)) return fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return 0;
}

}  // namespace

template <int D> void FullBaShared<D>::cost(const double* at, double* r_out, double* rho_out) { fba_cost(static_cast<Problem*>(this), at, r_out, rho_out); }
template <int D> void FullBaShared<D>::linearize() { fba_linearize(static_cast<Problem*>(this)); }
template <int D> int FullBaShared<D>::step(double radius, const gsfm_ba_options& o, BaStep* out) { return fba_step(static_cast<Problem*>(this), radius, o, out); }

extern "C" {

// ---- include/gsfm_ba6.h ---------------------------------------------------------------------------------------------------------------
int gsfm_ba6_abi_version(void) { return GSFM_BA6_ABI_VERSION; }

// gsfm_ba.h's defaults with the PCG tolerance two decades lower: see the header
void gsfm_ba6_options_default(gsfm_ba_options* o) {
  gsfm_ba_options_default(o);
  o->cg_relative_tolerance = 1e-14;
}

void gsfm_ba6_problem_destroy(gsfm_ba6_problem* P) { fba_destroy(P); }

gsfm_status gsfm_ba6_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                                    const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba6_problem** out) {
  return guarded("full bundle adjustment problem creation", fba_create_impl<gsfm_ba6_problem>, n_cams, intrinsics, cam_estimated, (const uint8_t*)nullptr, n_tracks,
                 track_ptr, obs_cam, obs_xy, point_estimated, out);
}

gsfm_status gsfm_ba6_set_loss(gsfm_ba6_problem* P, const gsfm_loss_node* prog, int32_t n) { return ba_set_loss(P, prog, n, "full bundle adjustment"); }

gsfm_status gsfm_ba6_solve(gsfm_ba6_problem* P, double* rot_aa, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  return guarded("the full bundle adjustment", fba_solve_impl<gsfm_ba6_problem>, P, rot_aa, cam_pos, (double*)nullptr, points, opt, summary);
}

gsfm_status gsfm_ba6_residuals(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  return guarded("full bundle adjustment residuals", fba_residuals_impl<gsfm_ba6_problem>, P, rot_aa, cam_pos, (const double*)nullptr, points, r_out, rho_out);
}

gsfm_status gsfm_ba6_linearize(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double* cost, double* grad_rot,
                               double* grad_pos, double* grad_point, double* diag_cam, double* diag_point) {
  return guarded("full bundle adjustment linearisation", fba_linearize_impl<gsfm_ba6_problem>, P, rot_aa, cam_pos, (const double*)nullptr, points, cost, grad_rot, grad_pos,
                 (double*)nullptr, grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_ba6_schur_matvec(gsfm_ba6_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  if (int st = fba_check_matvec(P, v, radius, y, "call gsfm_ba6_linearize or gsfm_ba6_step_check first")) return (gsfm_status)st;
  return guarded("full bundle adjustment Schur product", fba_schur_matvec_impl<gsfm_ba6_problem>, P, v, radius, opt, y);
}

gsfm_status gsfm_ba6_step_check(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, const gsfm_ba_options* opt,
                                double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out, double* delta_point_out,
                                double* jdelta_out, double* scal_out, int32_t* info_out) {
  if (int st = fba_check_point(P, FbaPoint{rot_aa, cam_pos, nullptr, points})) return (gsfm_status)st;
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("full bundle adjustment step check", fba_step_check_impl<gsfm_ba6_problem>, P, rot_aa, cam_pos, (const double*)nullptr, points, radius, opt, rhs_out, yc_out,
                 yp_out, delta_rot_out, delta_pos_out, (double*)nullptr, delta_point_out, jdelta_out, scal_out, info_out);
}

gsfm_status gsfm_ba6_time_kernels(gsfm_ba6_problem* P, const double* rot_aa, const double* cam_pos, const double* points, double radius, int32_t reps,
                                  double* out_us) {
  if (!P || !out_us) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = fba_check_point(P, FbaPoint{rot_aa, cam_pos, nullptr, points})) return (gsfm_status)st;
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  return guarded("full bundle adjustment kernel timing", fba_time_kernels_impl<gsfm_ba6_problem>, P, rot_aa, cam_pos, (const double*)nullptr, points, radius, reps, out_us);
}

// ---- include/gsfm_ba7.h ---------------------------------------------------------------------------------------------------------------
int gsfm_ba7_abi_version(void) { return GSFM_BA7_ABI_VERSION; }

// gsfm_ba6.h's defaults with a stall rule that looks further: see the header
void gsfm_ba7_options_default(gsfm_ba_options* o) {
  gsfm_ba6_options_default(o);
  o->cg_stall_iterations = o->max_cg_iterations / 2;
}

void gsfm_ba7_problem_destroy(gsfm_ba7_problem* P) { fba_destroy(P); }

gsfm_status gsfm_ba7_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, const uint8_t* focal_free, uint64_t n_tracks,
                                    const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                    gsfm_ba7_problem** out) {
  return guarded("focal-length bundle adjustment problem creation", fba_create_impl<gsfm_ba7_problem>, n_cams, intrinsics, cam_estimated, focal_free, n_tracks, track_ptr,
                 obs_cam, obs_xy, point_estimated, out);
}

gsfm_status gsfm_ba7_set_loss(gsfm_ba7_problem* P, const gsfm_loss_node* prog, int32_t n) { return ba_set_loss(P, prog, n, "focal-length bundle adjustment"); }

gsfm_status gsfm_ba7_solve(gsfm_ba7_problem* P, double* rot_aa, double* cam_pos, double* focal, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  return guarded("the focal-length bundle adjustment", fba_solve_impl<gsfm_ba7_problem>, P, rot_aa, cam_pos, focal, points, opt, summary);
}

gsfm_status gsfm_ba7_residuals(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* r_out,
                               double* rho_out) {
  return guarded("focal-length bundle adjustment residuals", fba_residuals_impl<gsfm_ba7_problem>, P, rot_aa, cam_pos, focal, points, r_out, rho_out);
}

gsfm_status gsfm_ba7_linearize(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* cost,
                               double* grad_rot, double* grad_pos, double* grad_focal, double* grad_point, double* diag_cam, double* diag_point) {
  return guarded("focal-length bundle adjustment linearisation", fba_linearize_impl<gsfm_ba7_problem>, P, rot_aa, cam_pos, focal, points, cost, grad_rot, grad_pos,
                 grad_focal, grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_ba7_schur_matvec(gsfm_ba7_problem* P, const double* v, double radius, const gsfm_ba_options* opt, double* y) {
  if (int st = fba_check_matvec(P, v, radius, y, "call gsfm_ba7_linearize or gsfm_ba7_step_check first")) return (gsfm_status)st;
  return guarded("focal-length bundle adjustment Schur product", fba_schur_matvec_impl<gsfm_ba7_problem>, P, v, radius, opt, y);
}

gsfm_status gsfm_ba7_step_check(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                const gsfm_ba_options* opt, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out, double* delta_pos_out,
                                double* delta_focal_out, double* delta_point_out, double* jdelta_out, double* scal_out, int32_t* info_out) {
  if (int st = fba_check_point(P, FbaPoint{rot_aa, cam_pos, focal, points})) return (gsfm_status)st;
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  return guarded("focal-length bundle adjustment step check", fba_step_check_impl<gsfm_ba7_problem>, P, rot_aa, cam_pos, focal, points, radius, opt, rhs_out, yc_out, yp_out,
                 delta_rot_out, delta_pos_out, delta_focal_out, delta_point_out, jdelta_out, scal_out, info_out);
}

gsfm_status gsfm_ba7_time_kernels(gsfm_ba7_problem* P, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                  int32_t reps, double* out_us) {
  if (!P || !out_us) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = fba_check_point(P, FbaPoint{rot_aa, cam_pos, focal, points})) return (gsfm_status)st;
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  return guarded("focal-length bundle adjustment kernel timing", fba_time_kernels_impl<gsfm_ba7_problem>, P, rot_aa, cam_pos, focal, points, radius, reps, out_us);
}

}  // extern "C"
