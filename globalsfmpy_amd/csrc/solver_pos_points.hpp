// Host side of camera-position estimation with point-to-camera constraints (include/gsfm_posp.h): the sum of the position problem
// (solver_pos.hpp: the edge CSR, the world directions, the loss program) and of the bundle problem's point elimination (solver_ba.hpp:
// BaProblem with the structure arrays, the vectors of the step, BaLm for lm_loop.hpp's Levenberg-Marquardt loop, the lane-class launcher
// and the checks of track_scene.hpp).  Its own: problem creation over both structures, the reduced camera operator that carries the edge
// Laplacian and the Schur term (posp_schur_product), its PCG on lm_loop.hpp's driver, and the step with gsfm_pos.h's scale gauge over
// cameras and points.  The kernels are pos_point_kernels.hpp's; the point pass, the quadratic form over tracks, the points' inverses and
// the vector kernels are ba_kernels.hpp's and pos_kernels.hpp's.  The public options are gsfm_pos_options; inside, the loop runs on their
// gsfm_ba_options image (the same fields but dense_max_cams, which this solver ignores).
// Memory: one slab laid out by FlatLayout and owned, with the problem's private non-blocking stream, by BaProblem's FlatCall member.
#pragma once
#include "solver_pos.hpp"
#include "solver_ba.hpp"
#include "pos_point_kernels.hpp"
#include "../../include/gsfm_posp.h"

struct gsfm_posp_problem : BaProblem {
  // observation side, ba_kernels.hpp's layouts
  double *Ht = nullptr, *At = nullptr, *Hc = nullptr, *v = nullptr, *Cfix = nullptr;
  uint8_t *cam_used = nullptr, *obs_used = nullptr;
  double *ray = nullptr, *ray_aa = nullptr, *intr = nullptr;
  double w_p = 0.5;
  // edge side, pos_kernels.hpp's layouts
  uint64_t n_edges = 0;
  std::vector<uint8_t> present;             // camera appears in an edge
  uint32_t *row_ptr = nullptr, *nbr = nullptr, *eid = nullptr, *ei = nullptr, *ej = nullptr;
  double *dir_k = nullptr, *dir_e = nullptr, *H = nullptr;
  // loss (gsfm_pos_set_loss's programs)
  DevLoss* d_loss = nullptr;
  DevBuf<double> tables[3];
  int lm = LM_SIMPLE;
  int32_t fixed = -1;                       // the camera held constant by the call that is running
  void cost(const double* at, double* r_out, double* rho_out) override;
  void linearize() override;
  int step(double radius, const gsfm_ba_options& o, BaStep* out) override;
};

namespace {

// the device scalars beyond BaLm's: the edge and the track part of the cost and of the quadratic form
enum { PP_COST_E = BS_N, PP_COST_T, PP_DLD_E, PP_DLD_T, PP_N };

PosDev posp_edges(const gsfm_posp_problem* P) {
  PosDev a{};
  a.n_cams = P->n_cams; a.n_edges = (uint32_t)P->n_edges;
  a.row_ptr = P->row_ptr; a.nbr = P->nbr; a.eid = P->eid; a.dir_k = P->dir_k; a.ei = P->ei; a.ej = P->ej; a.dir_e = P->dir_e;
  a.active = P->active; a.H = P->H; a.loss = P->d_loss; a.rho_ext = nullptr;
  return a;
}
BaDev posp_dev(const gsfm_posp_problem* P) {
  BaDev a = ba_dev_shared(P);
  a.Ht = P->Ht; a.At = P->At; a.Hc = P->Hc;
  return a;
}
gsfm::PpObs posp_obs(const gsfm_posp_problem* P) { return {P->cam_used, P->ray, P->w_p, P->d_loss}; }

// a track-side kernel of pos_point_kernels.hpp over every track, in the specialisation of the problem's loss
#define PP_TRACKS(P, K, ...)                                                                                                              \
  ((P)->lm == LM_SIMPLE ? ba_tracks(P, posp_dev(P), K<4, LM_SIMPLE>, K<16, LM_SIMPLE>, K<64, LM_SIMPLE>, posp_obs(P), __VA_ARGS__)        \
                        : ba_tracks(P, posp_dev(P), K<4, LM_PROGRAM>, K<16, LM_PROGRAM>, K<64, LM_PROGRAM>, posp_obs(P), __VA_ARGS__))
#define PP_BA_TRACKS(P, K, ...) ba_tracks(P, posp_dev(P), K<4>, K<16>, K<64>, __VA_ARGS__)

// cost of the point `at` into scal[BS_COST]: the edge sum (k_pos_cost) plus the track sum
void posp_cost(gsfm_posp_problem* P, const double* at, double* r_out, double* rho_out) {
  const DevScalars V = P->vec();
  hipLaunchKernelGGL(P->lm == LM_SIMPLE ? k_pos_cost<LM_SIMPLE> : k_pos_cost<LM_PROGRAM>, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, posp_edges(P), at, P->part);
  V.reduce(PP_COST_E);
  PP_TRACKS(P, k_pp_cost_tracks, at, P->pt_scratch, r_out, rho_out);
  ba_sum(P, P->pt_scratch, P->n_tracks, PP_COST_T);
  hipLaunchKernelGGL(k_pp_add, dim3(1), dim3(64), 0, P->mem.s, P->scal, (int)PP_COST_E, (int)PP_COST_T, (int)BS_COST);
}
// linearisation at P->x: the track side evaluates every observation, the camera rows evaluate their edge entries and sum both
void posp_linearize(gsfm_posp_problem* P) {
  PP_TRACKS(P, k_pp_lin_tracks, (const double*)P->x, P->g, P->Dg);
  hipLaunchKernelGGL(P->lm == LM_SIMPLE ? k_pp_cam_lin<LM_SIMPLE> : k_pp_cam_lin<LM_PROGRAM>, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P),
                     (const double*)P->x, P->g, P->Dg);
}

// D^2 at the radius, b = S g, the points' inverses (ba_kernels.hpp's, with their second tier)
void posp_prep(gsfm_posp_problem* P, double radius, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_ba_prep_nodes, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, P->n_nodes, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal,
                     o.max_lm_diagonal, P->D2, P->b);
  hipLaunchKernelGGL(k_ba_prep_points, ba_grid(P->n_tracks), dim3(256), 0, P->mem.s, P->n_cams, P->n_tracks, P->active, P->Dg, P->S, P->D2, P->b, P->Cinv, P->Cfix, P->Gt,
                     P->zt);
}
// out = Sc v on the cameras, v = pvec and q = S pvec given: the point pass, then the camera pass over edges and observations
void posp_schur_product(gsfm_posp_problem* P, const double* qvec, const double* pvec, double* out) {
  PP_BA_TRACKS(P, k_ba_point_pass, qvec, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)nullptr, P->zt, 1);
  hipLaunchKernelGGL(k_pp_cam_pass, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P), qvec, (const double*)P->zt, pvec, (const double*)P->S,
                     (const double*)P->D2, (const double*)nullptr, out, 1);
}
void posp_precond(gsfm_posp_problem* P) {
  hipLaunchKernelGGL(k_pp_cam_precond, ba_row_grid(P->n_cams), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P), (const double*)P->S, (const double*)P->D2,
                     (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Cfix, P->Minv);
}

// PCG on Sc y_c = rhs from y_c = 0 (k_ba_pcg_init set r, z, p, q): lm_loop.hpp's driver, with the breakdown rule of the bundle adjustments
int posp_pcg(gsfm_posp_problem* P, const gsfm_ba_options& o, BaStep* out) {
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams;
  V.dot(P->r, P->z, nullptr, N, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    posp_schur_product(P, P->q, P->p, P->Ap);
    V.dot(P->p, P->Ap, nullptr, N, BS_PAP);
    hipLaunchKernelGGL(k_pos_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, N, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, true, iterate, V.pcg_reader(), &out->cg, &out->stalled, &out->cg_rel);
}

// One LM step's linear algebra at P->x, after its linearisation and with the Jacobi scale in place -- shared by the solve and by
// gsfm_posp_step_check.  Leaves y (cameras, then points), delta, the trial point P->cand and scal[BS_STEP2], [BS_DG], [BS_DLD] enqueued.
int posp_step(gsfm_posp_problem* P, double radius, const gsfm_ba_options& o, BaStep* out) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes;
  const DevScalars V = P->vec();
  *out = BaStep();
  posp_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the preconditioner, the PCG start
  hipLaunchKernelGGL(k_pp_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P), (const double*)nullptr, (const double*)P->zt, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  posp_precond(P);
  hipLaunchKernelGGL(k_ba_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = posp_pcg(P, o, out)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N), dim3(256), 0, P->mem.s, (size_t)N, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) PP_BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)P->b, P->y + 3 * (size_t)N, 0);
  // the step over cameras and points, its scale-gauge part about the fixed camera removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_pos_step, ba_grid(NN), dim3(256), 0, P->mem.s, (uint32_t)NN, P->active, P->S, P->y, P->x, P->fixed, o.remove_gauge, P->delta, P->v);
  V.dot(P->delta, P->v, nullptr, NN, BS_DV);
  V.dot(P->v, P->v, nullptr, NN, BS_VV);
  hipLaunchKernelGGL(k_pos_project, ba_grid(NN), dim3(256), 0, P->mem.s, (uint32_t)NN, P->scal, BS_DV, BS_VV, P->v, P->delta, P->x, P->cand);
  V.dot(P->delta, P->delta, nullptr, NN, BS_STEP2);
  V.dot(P->delta, P->g, nullptr, NN, BS_DG);
  // delta^T (J~^T J~) delta: the edges' part by the position problem's product, the tracks' part by the bundle problem's quadratic form
  hipLaunchKernelGGL(k_pos_matvec<false>, ba_row_grid(N), dim3(256), 0, P->mem.s, posp_edges(P), (const double*)P->delta, (const double*)P->delta, (const double*)P->S,
                     (const double*)P->D2, P->Ap);
  V.dot(P->delta, P->Ap, nullptr, N, PP_DLD_E);
  PP_BA_TRACKS(P, k_ba_quad_tracks, (const double*)P->delta, P->pt_scratch);
  ba_sum(P, P->pt_scratch, T, PP_DLD_T);
  hipLaunchKernelGGL(k_pp_add, dim3(1), dim3(64), 0, P->mem.s, P->scal, (int)PP_DLD_E, (int)PP_DLD_T, (int)BS_DLD);
  return 0;
}

// the loop's options: gsfm_pos_options' fields under gsfm_ba_options' names (dense_max_cams has no counterpart: every step is PCG)
gsfm_ba_options posp_options(const gsfm_pos_options* opt) {
  const gsfm_pos_options p = pos_options(opt);
  gsfm_ba_options o;
  std::memset(&o, 0, sizeof(o));
  o.max_num_iterations = p.max_num_iterations; o.jacobi_scaling = p.jacobi_scaling;
  o.function_tolerance = p.function_tolerance; o.gradient_tolerance = p.gradient_tolerance; o.parameter_tolerance = p.parameter_tolerance;
  o.initial_trust_region_radius = p.initial_trust_region_radius; o.max_trust_region_radius = p.max_trust_region_radius;
  o.min_trust_region_radius = p.min_trust_region_radius; o.min_relative_decrease = p.min_relative_decrease;
  o.min_lm_diagonal = p.min_lm_diagonal; o.max_lm_diagonal = p.max_lm_diagonal;
  o.max_cg_iterations = p.max_cg_iterations; o.cg_check_interval = p.cg_check_interval; o.cg_relative_tolerance = p.cg_relative_tolerance;
  o.cg_stall_iterations = p.cg_stall_iterations; o.remove_gauge = p.remove_scale_gauge; o.verbose = p.verbose;
  return o;
}

bool posp_needs_points(const gsfm_posp_problem* P, const double* cam_pos, const double* points) { return !cam_pos || (P->n_tracks > 0 && !points); }
// fixed_cam is -1 or a camera that appears in an edge
int posp_check_fixed(const gsfm_posp_problem* P, int32_t fixed_cam) {
  if (fixed_cam >= -1 && fixed_cam < (int64_t)P->n_cams && (fixed_cam < 0 || P->present[fixed_cam])) return 0;
  return fail(GSFM_ERR_INVALID_ARG, "fixed_cam must be -1 or a camera that appears in an edge");
}
// The active set (the cameras of the edges less fixed_cam, the active points) and x = (cam_pos, points), enqueued
int posp_upload_point(gsfm_posp_problem* P, const double* cam_pos, const double* points, int32_t fixed_cam) {
  const size_t N = P->n_cams, T = P->n_tracks;
  std::copy(P->present.begin(), P->present.end(), P->h_active.begin());
  if (fixed_cam >= 0) P->h_active[fixed_cam] = 0;
  P->fixed = fixed_cam;
  HIPCHK(hipMemcpyAsync(P->active, P->h_active.data(), P->n_nodes, hipMemcpyHostToDevice, P->mem.s));
  HIPCHK(hipMemcpyAsync(P->x, cam_pos, 24 * N, hipMemcpyHostToDevice, P->mem.s));
  if (T) HIPCHK(hipMemcpyAsync(P->x + 3 * N, points, 24 * T, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}

// The arrays of the slab in order.  *zeroed: the bytes one memset clears.
FlatLayout posp_place(gsfm_posp_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes, E = P->n_edges, ND = 2 * E;
  SlabTake take{FlatLayout(), slab};
  take(P->scal, PP_N); take(P->Dg, 6 * NN);
  take(P->d_loss, 1);   // (all zeros: Ceres' NULL loss, the state of a new problem)
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta, &P->v}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 3 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Cfix, GSFM_BA_FIX_DOUBLES * T);   // (no point is flagged before the first k_ba_prep_points)
  *zeroed = take.L.total;
  take(P->Minv, 9 * N); take(P->Cinv, 9 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS);
  take(P->Ht, 6 * O); take(P->At, 3 * O); take(P->Hc, 6 * U); take(P->ray, 3 * O); take(P->ray_aa, 3 * N); take(P->intr, 3 * N);
  take(P->dir_k, 3 * ND); take(P->dir_e, 3 * E); take(P->H, 6 * ND);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->row_ptr, N + 1); take(P->nbr, ND); take(P->eid, ND); take(P->ei, E); take(P->ej, E);
  take(P->track_used, T); take(P->active, NN); take(P->cam_used, N); take(P->obs_used, O);
  return take.L;
}

// The checks of create, on the host before any device call: gsfm_pos_problem_create's, the weight, gsfm_ba_problem_create's
int posp_check_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
                      const double* ray_rot_aa, const double* intrinsics, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                      double weight) {
  if (n_cams == 0 || n_edges == 0) return fail(GSFM_ERR_EMPTY, "no cameras or no edges");
  if (!edge_i || !edge_j || !rel_t || !rot_aa) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31) || n_cams >= (1u << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges or cameras)");
  for (uint64_t e = 0; e < n_edges; ++e)
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams || edge_i[e] == edge_j[e]) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has a bad camera index");
  if (!(weight > 0.0) || !std::isfinite(weight)) return fail(GSFM_ERR_INVALID_ARG, "point_to_camera_weight must be finite and positive");
  if (int st = track_arrays_check(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, TrackLimit::observations_and_nodes, n_cams,
                                  "NULL argument (track_ptr holds n_tracks + 1 entries)")) return st;
  if (track_ptr[n_tracks] > 0 && (!ray_rot_aa || !intrinsics)) return fail(GSFM_ERR_INVALID_ARG, "NULL argument (ray_rot_aa and intrinsics are read when there are observations)");
  if (const char* why = no_device_reason("gsfm_posp_problem_create")) return fail(GSFM_ERR_NO_DEVICE, why);
  return 0;
}

gsfm_status posp_create_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
                             const double* ray_rot_aa, const double* intrinsics, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                             const double* obs_xy, double weight, gsfm_posp_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  const uint64_t no_tracks[1] = {0};
  if (n_tracks == 0 && !track_ptr) track_ptr = no_tracks;
  if (int st = posp_check_create(n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa, ray_rot_aa, intrinsics, n_tracks, track_ptr, obs_cam, obs_xy, weight)) return (gsfm_status)st;
  const size_t N = n_cams, E = n_edges, T = n_tracks, O = track_ptr[n_tracks];
  // host structures and upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  PosStructure S = pos_build_structure(n_cams, n_edges, edge_i, edge_j);
  // a point is active with two or more observations in cameras of the edges; an observation is used when its camera is one and its point is active
  std::vector<uint8_t> two_views(T, 0), obs_used(O, 0);
  for (size_t t = 0; t < T; ++t) {
    uint64_t n = 0;
    for (uint64_t e = track_ptr[t]; e < track_ptr[t + 1]; ++e) n += S.present[obs_cam[e]];
    two_views[t] = n >= 2;
    if (two_views[t]) for (uint64_t e = track_ptr[t]; e < track_ptr[t + 1]; ++e) obs_used[e] = S.present[obs_cam[e]];
  }
  hvec<uint32_t> order(T);
  PosTmp tmp(N, E);
  std::unique_ptr<gsfm_posp_problem, void (*)(gsfm_posp_problem*)> P(new gsfm_posp_problem, gsfm_posp_problem_destroy);
  ba_init(P.get(), n_cams, 1, S.present.data(), n_tracks, track_ptr, obs_cam, two_views.data(), order.data());
  P->n_edges = n_edges; P->w_p = weight; P->present = S.present;
  std::copy(S.present.begin(), S.present.end(), P->h_active.begin());   // (every camera of the edges; a call sets its fixed camera)
  if (tmp.buf.alloc(tmp.L.total) != hipSuccess) { (void)hipGetLastError(); return (gsfm_status)fail(GSFM_ERR_HIP, "allocating the upload buffers of the position problem failed"); }
  size_t zeroed = 0;
  if (int st = ba_commit_upload(P.get(), posp_place, "the position problem with points", track_ptr, order.data(), obs_cam, obs_xy, &zeroed)) return (gsfm_status)st;
  const hipStream_t s = P->mem.s;
  HIPCHK_S(ba_up(s, P->row_ptr, S.row_ptr.data(), 4 * (N + 1))); HIPCHK_S(ba_up(s, P->nbr, S.nbr.data(), 8 * E)); HIPCHK_S(ba_up(s, P->eid, S.eid.data(), 8 * E));
  HIPCHK_S(ba_up(s, P->ei, edge_i, 4 * E)); HIPCHK_S(ba_up(s, P->ej, edge_j, 4 * E));
  HIPCHK_S(ba_up(s, tmp.ptr(tmp.pos_i), S.pos_i.data(), 4 * E)); HIPCHK_S(ba_up(s, tmp.ptr(tmp.pos_j), S.pos_j.data(), 4 * E));
  HIPCHK_S(ba_up(s, tmp.ptr(tmp.rel), rel_t, 24 * E)); HIPCHK_S(ba_up(s, tmp.ptr(tmp.rot), rot_aa, 24 * N));
  hipLaunchKernelGGL(k_pos_directions, ba_grid(E), dim3(256), 0, s, (uint32_t)E, P->ei, (const double*)tmp.ptr(tmp.rot), (const double*)tmp.ptr(tmp.rel),
                     (const uint32_t*)tmp.ptr(tmp.pos_i), (const uint32_t*)tmp.ptr(tmp.pos_j), P->dir_e, P->dir_k);
  HIPCHK_S(ba_up(s, P->cam_used, S.present.data(), N)); HIPCHK_S(ba_up(s, P->obs_used, obs_used.data(), O));
  if (O > 0) {
    HIPCHK_S(ba_up(s, P->ray_aa, ray_rot_aa, 24 * N)); HIPCHK_S(ba_up(s, P->intr, intrinsics, 24 * N));
    hipLaunchKernelGGL(k_pp_rays, ba_grid(O), dim3(256), 0, s, (uint64_t)O, (const uint32_t*)P->obs_cam, (const double2*)P->obs_xy, (const uint8_t*)P->obs_used,
                       (const double*)P->ray_aa, (const double*)P->intr, P->ray);
  }
  if (int st = sync_stream(s, "position problem with points create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

void posp_scatter(const gsfm_posp_problem* P, const double* xh, double* cam_pos, double* points) {
  const size_t N = P->n_cams, T = P->n_tracks;
  for (size_t k = 0; k < N; ++k) if (P->h_active[k]) std::copy(&xh[3 * k], &xh[3 * k] + 3, cam_pos + 3 * k);
  for (size_t t = 0; t < T; ++t) if (P->h_active[N + t]) std::copy(&xh[3 * (N + t)], &xh[3 * (N + t)] + 3, points + 3 * t);
}

gsfm_status posp_solve_impl(gsfm_posp_problem* P, double* cam_pos, double* points, int32_t fixed_cam, const gsfm_pos_options* opt, gsfm_posp_summary* summary) {
  if (!P || posp_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = posp_check_fixed(P, fixed_cam)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const gsfm_ba_options o = posp_options(opt);
  gsfm_posp_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->pos.num_edges_used = P->n_edges; summary->num_observations_used = P->n_used; summary->num_active_points = P->st.n_active_points;
  const double t0 = now_ms();
  if (int st = posp_upload_point(P, cam_pos, points, fixed_cam)) return (gsfm_status)st;
  gsfm_ba_summary bs;
  std::memset(&bs, 0, sizeof(bs));
  BaLm ops{P, o, &bs, {}};
  if (int st = lm_loop(ops, o, &bs, "posp")) return (gsfm_status)st;
  hvec<double> xh(3 * P->n_nodes);
  if (int st = P->vec().read(xh.data(), P->x, 24 * P->n_nodes, "download the estimates")) return (gsfm_status)st;
  posp_scatter(P, xh.data(), cam_pos, points);
  gsfm_pos_summary& s = summary->pos;
  s.termination = bs.termination; s.num_iterations = bs.num_iterations; s.num_successful_steps = bs.num_successful_steps;
  s.num_unsuccessful_steps = bs.num_unsuccessful_steps; s.num_cg_iterations = bs.num_cg_iterations; s.num_pcg_stalled_steps = bs.num_pcg_stalled_steps;
  s.num_residual_sweeps = bs.num_residual_sweeps; s.num_linearizations = bs.num_linearizations; s.nonfinite = bs.nonfinite;
  s.initial_cost = bs.initial_cost; s.final_cost = bs.final_cost; s.final_gradient_max_norm = bs.final_gradient_max_norm;
  s.final_radius = bs.final_radius; s.max_radius = bs.max_radius;
  s.t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status posp_linearize_impl(gsfm_posp_problem* P, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                                double* diag_cam, double* diag_point) {
  if (!P || posp_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = N + T;
  double c = 0.0;
  if (int st = posp_upload_point(P, cam_pos, points, -1)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, posp_options(nullptr), &c)) return (gsfm_status)st;
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

gsfm_status posp_residuals_impl(gsfm_posp_problem* P, const double* cam_pos, const double* points, double* r_edge, double* rho_edge, double* r_obs, double* rho_obs,
                                double* ray_out) {
  if (!P || posp_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t E = P->n_edges, O = P->n_obs;
  FlatLayout L;
  const Slot<double> re = L.take<double>(3 * E), rhe = L.take<double>(E), ro = L.take<double>(3 * O), rho = L.take<double>(O);
  DevBuf<char> scratch;
  if (scratch.alloc(L.total) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  auto at = [&](Slot<double> h) { return (double*)(scratch.p + h.off); };
  if (int st = posp_upload_point(P, cam_pos, points, P->fixed)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_pos_resid, ba_grid(E), dim3(256), 0, P->mem.s, posp_edges(P), (const double*)P->x, at(re), (double*)nullptr, at(rhe), 1);
  posp_cost(P, P->x, at(ro), at(rho));
  auto down = [&](double* dst, const double* src, size_t n) { return (dst && n) ? hipMemcpyAsync(dst, src, 8 * n, hipMemcpyDeviceToHost, P->mem.s) : hipSuccess; };
  HIPCHK_S(down(r_edge, at(re), 3 * E)); HIPCHK_S(down(rho_edge, at(rhe), E)); HIPCHK_S(down(r_obs, at(ro), 3 * O)); HIPCHK_S(down(rho_obs, at(rho), O));
  HIPCHK_S(down(ray_out, P->ray, 3 * O));
  return (gsfm_status)sync_stream(P->mem.s, "residuals");
}

}  // namespace

void gsfm_posp_problem::cost(const double* at, double* r_out, double* rho_out) { posp_cost(this, at, r_out, rho_out); }
void gsfm_posp_problem::linearize() { posp_linearize(this); }
int gsfm_posp_problem::step(double radius, const gsfm_ba_options& o, BaStep* out) { return posp_step(this, radius, o, out); }

extern "C" {

int gsfm_posp_abi_version(void) { return GSFM_POSP_ABI_VERSION; }

void gsfm_posp_problem_destroy(gsfm_posp_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

gsfm_status gsfm_posp_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
                                     const double* ray_rot_aa, const double* intrinsics, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                     const double* obs_xy, double point_to_camera_weight, gsfm_posp_problem** out) {
  return guarded("creation of the position problem with points", posp_create_impl, n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa, ray_rot_aa, intrinsics, n_tracks,
                 track_ptr, obs_cam, obs_xy, point_to_camera_weight, out);
}

gsfm_status gsfm_posp_set_loss(gsfm_posp_problem* P, const gsfm_loss_node* prog, int32_t n) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  DevLoss L;
  if (int st = build_dev_loss(prog, n, P->tables, P->mem.s, L)) return (gsfm_status)st;
  bool simple = n == 0;
  if (n == 1) {
    const int k = prog[0].kind;
    simple = k == GSFM_LOSS_TRIVIAL || k == GSFM_LOSS_HUBER || k == GSFM_LOSS_SOFT_L1 || k == GSFM_LOSS_TUKEY || k == GSFM_LOSS_GEMAN_MCCLURE;
  }
  P->lm = simple ? LM_SIMPLE : LM_PROGRAM;
  P->have_lin = false;
  HIPCHK_S(hipMemcpyAsync(P->d_loss, &L, sizeof(L), hipMemcpyHostToDevice, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "set_loss");
}

gsfm_status gsfm_posp_set_loss_callback(gsfm_posp_problem*, gsfm_loss_callback, void*) {
  return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "a host-callback loss is not supported with point-to-camera constraints (use a loss with a native program, or gsfm_pos.h without tracks)");
}

gsfm_status gsfm_posp_solve(gsfm_posp_problem* P, double* cam_pos, double* points, int32_t fixed_cam, const gsfm_pos_options* opt, gsfm_posp_summary* summary) {
  return guarded("the position solve with points", posp_solve_impl, P, cam_pos, points, fixed_cam, opt, summary);
}

gsfm_status gsfm_posp_residuals(gsfm_posp_problem* P, const double* cam_pos, const double* points, double* r_edge_out, double* rho_edge_out, double* r_obs_out,
                                double* rho_obs_out, double* ray_out) {
  return guarded("position residuals with points", posp_residuals_impl, P, cam_pos, points, r_edge_out, rho_edge_out, r_obs_out, rho_obs_out, ray_out);
}

gsfm_status gsfm_posp_linearize(gsfm_posp_problem* P, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                                double* diag_cam, double* diag_point) {
  return guarded("position linearisation with points", posp_linearize_impl, P, cam_pos, points, cost, grad_cam, grad_point, diag_cam, diag_point);
}

gsfm_status gsfm_posp_schur_matvec(gsfm_posp_problem* P, const double* v, double radius, const gsfm_pos_options* opt, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_posp_linearize or gsfm_posp_step_check first");
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = posp_options(opt);
  const size_t N = P->n_cams;
  ba_jacobi_scale(P, o);
  posp_prep(P, radius, o);
  HIPCHK_S(hipMemcpyAsync(P->p, v, 24 * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->S, P->p, 1.0, P->q);
  posp_schur_product(P, P->q, P->p, P->Ap);
  HIPCHK_S(hipMemcpyAsync(y, P->Ap, 24 * N, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "schur_matvec");
}

gsfm_status gsfm_posp_step_check(gsfm_posp_problem* P, const double* cam_pos, const double* points, int32_t fixed_cam, double radius, const gsfm_pos_options* opt,
                                 double* rhs_out, double* yc_out, double* yp_out, double* delta_cam_out, double* delta_point_out, double* scal_out, int32_t* info_out) {
  if (!P || posp_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = posp_check_fixed(P, fixed_cam)) return (gsfm_status)st;
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  const gsfm_ba_options o = posp_options(opt);
  const size_t N = P->n_cams, T = P->n_tracks;
  double cost = 0.0;
  if (int st = posp_upload_point(P, cam_pos, points, fixed_cam)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
  BaStep step;
  if (int st = posp_step(P, radius, o, &step)) return (gsfm_status)st;
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

gsfm_status gsfm_posp_time_kernels(gsfm_posp_problem* P, const double* cam_pos, const double* points, double radius, int32_t reps, double* out_us) {
  if (!P || !out_us || posp_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0) || reps < 1) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius and reps must be positive");
  DeviceGuard g(P->device);
  gsfm_ba_options o = posp_options(nullptr);
  double cost = 0.0;
  if (int st = posp_upload_point(P, cam_pos, points, -1)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = posp_step(P, radius, o, &step)) return (gsfm_status)st;
  KernelTimer timed{P->mem.s, reps, out_us};
  if (int st = timed.create()) return (gsfm_status)st;
  const uint32_t N = P->n_cams;
  const size_t O = P->n_obs;
  timed([&] { if (O > 0) hipLaunchKernelGGL(k_pp_rays, ba_grid(O), dim3(256), 0, P->mem.s, (uint64_t)O, (const uint32_t*)P->obs_cam, (const double2*)P->obs_xy,
                                            (const uint8_t*)P->obs_used, (const double*)P->ray_aa, (const double*)P->intr, P->ray); });
  timed([&] { PP_TRACKS(P, k_pp_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(P->lm == LM_SIMPLE ? k_pp_cam_lin<LM_SIMPLE> : k_pp_cam_lin<LM_PROGRAM>, ba_row_grid(N), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P),
                                 (const double*)P->x, P->g, P->Dg); });
  timed([&] { PP_TRACKS(P, k_pp_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { PP_BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)nullptr, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_pp_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, posp_edges(P), posp_dev(P), (const double*)P->q, (const double*)P->zt,
                                 (const double*)P->p, (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { posp_precond(P); });
  return (gsfm_status)timed.st;
}

}  // extern "C"
