// Host side of the bundle adjustment of camera positions and points (include/gsfm_ba.h), and what it shares with the full bundle adjustment
// (solver_full_ba.hpp): the problem's common part (BaProblem: sizes, host structure of ba_structure.hpp, structure arrays, the vectors of the
// step), the operations that lm_loop.hpp's Levenberg-Marquardt loop runs (BaLm), argument checks, set_loss, solve, residuals and kernel
// timing; the checks of the track arrays, the lane classes with their launcher and the one-leaf loss are track_scene.hpp's.  Its own: the
// Schur-complement PCG (ba_pcg, on lm_loop.hpp's driver) and the step.  The kernels are in ba_kernels.hpp; the vector kernels of the PCG
// and the reductions are the position problem's (pos_kernels.hpp, dev_scalars.hpp), which work on any n x 3 array.
// Memory: one slab laid out by FlatLayout and owned, with the problem's private non-blocking stream, by a FlatCall member (flat_call.hpp).
// Every copy and memset is ordered on that stream.  The unknowns are one array of (n_cams + n_tracks) x 3, cameras first.
#pragma once
#include "host_common.hpp"
#include "flat_call.hpp"
#include "ba_structure.hpp"
#include "lm_loop.hpp"
#include "dev_scalars.hpp"
#include "track_scene.hpp"
#include "ba_kernels.hpp"
#include "../../include/gsfm_ba.h"

#include <memory>

struct BaStep { int cg = 0; bool stalled = false; double cg_rel = 0.0; };

// What both bundle adjustments have.  A camera is one node of 3 doubles here and two or three (angle-axis vector, centre, intrinsics) in solver_full_ba.hpp.
struct BaProblem {
  int device = 0;
  FlatCall mem;
  uint32_t n_cams = 0, n_tracks = 0;
  uint64_t n_obs = 0, n_used = 0;
  size_t n_nodes = 0;
  uint64_t n_active = 0;                     // active cameras + active points (the nodes the gauge's centroid runs over)
  uint64_t cb[4] = {0, 0, 0, 0};             // the lane classes' slices of the launch order
  BaStructure st;                            // host copy of the active sets
  std::vector<uint8_t> h_active;             // n_nodes
  gsfm::DevLossNode leaf;
  // device arrays (ba_place / fba_place): the structure
  uint32_t *order = nullptr, *obs_cam = nullptr, *crow_ptr = nullptr, *cobs = nullptr, *ctrk = nullptr;
  uint64_t* track_ptr = nullptr;
  double2* obs_xy = nullptr;
  uint8_t *track_used = nullptr, *active = nullptr;
  double* cams = nullptr;
  // per node (3 or 6 doubles each)
  double *x = nullptr, *cand = nullptr, *g = nullptr, *Dg = nullptr, *S = nullptr, *D2 = nullptr, *b = nullptr, *y = nullptr, *delta = nullptr;
  // per camera node
  double *rhs = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *Ap = nullptr, *Minv = nullptr;
  // per point
  double *Cinv = nullptr, *Gt = nullptr, *zt = nullptr, *pt_scratch = nullptr;
  double *part = nullptr, *scal = nullptr;
  bool have_lin = false;

  virtual ~BaProblem() = default;
  DevScalars vec() const { return {mem.s, part, scal}; }
  // where the two solvers differ, for the code they share:
  virtual void cost(const double* at, double* r_out, double* rho_out) = 0;          // cost of the point `at` into scal[BS_COST]
  virtual void linearize() = 0;                                                     // linearisation at x
  virtual int step(double radius, const gsfm_ba_options& o, BaStep* out) = 0;       // one LM step's linear algebra (ba_step / fba_step)
};

struct gsfm_ba_problem : BaProblem {
  double *Ht = nullptr, *At = nullptr, *Hc = nullptr;   // per observation
  double* v = nullptr;                                   // per node
  double* Cfix = nullptr;                                // per point
  void cost(const double* at, double* r_out, double* rho_out) override;
  void linearize() override;
  int step(double radius, const gsfm_ba_options& o, BaStep* out) override;
};

namespace {

using gsfm::BaDev;
using gsfm::BaSlots;

// the device scalars of both solvers (solver_full_ba.hpp's further ones follow BS_N)
enum { BS_RZ0 = PCG_RZ0, BS_RZA = PCG_RZA, BS_RZB = PCG_RZB, BS_PAP = 3, BS_DV = 4, BS_VV = 5, BS_STEP2 = 6, BS_DG = 7, BS_DLD = 8, BS_COST = 9,
       BS_GMAX = 10, BS_XNORM2 = 11, BS_SUMD = 12 /* 3 */, BS_SUMX = 15 /* 3 */, BS_N = 18 };

// the kernel arguments that both solvers fill
BaDev ba_dev_shared(const BaProblem* P) {
  BaDev a{};
  a.n_cams = P->n_cams; a.n_tracks = P->n_tracks;
  a.track_ptr = P->track_ptr; a.obs_cam = P->obs_cam; a.obs_xy = P->obs_xy; a.cams = P->cams; a.track_used = P->track_used;
  a.crow_ptr = P->crow_ptr; a.cobs = P->cobs; a.ctrk = P->ctrk; a.active = P->active; a.leaf = P->leaf;
  return a;
}
BaDev ba_dev(const gsfm_ba_problem* P) {
  BaDev a = ba_dev_shared(P);
  a.Ht = P->Ht; a.At = P->At; a.Hc = P->Hc;
  return a;
}
// (at least one block: an empty launch is an error, and every kernel checks its bound)
inline dim3 ba_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + 255) / 256)); }
inline dim3 ba_row_grid(uint32_t n_cams) { return dim3(std::max(1u, (n_cams + 3) / 4)); }

// a point-side kernel over every track: one launch per lane class, the long tracks first (track_scene.hpp's launcher).  a: BaDev or FbaDev
template <typename Dev, typename K, typename... Args>
void ba_tracks(const BaProblem* P, const Dev& a, K k4, K k16, K k64, Args... args) {
  for_lane_classes(P->cb, [&](auto G, uint64_t n_slots, uint64_t offset, dim3 grid, dim3 block) {
    const BaSlots sl{n_slots, P->order + offset};
    hipLaunchKernelGGL(G() == 64 ? k64 : G() == 16 ? k16 : k4, grid, block, 0, P->mem.s, a, sl, args...);
  });
}
#define BA_TRACKS(P, K, ...) ba_tracks(P, ba_dev(P), K<4>, K<16>, K<64>, __VA_ARGS__)

// scal[slot] = the sum of a's n entries, in a fixed order
void ba_sum(const BaProblem* P, const double* a, size_t n, int slot) {
  hipLaunchKernelGGL(k_ba_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, a, n, P->part);
  P->vec().reduce(slot);
}
void ba_norms(const BaProblem* P) { P->vec().norms(P->g, P->x, P->active, P->n_nodes, BS_GMAX, BS_XNORM2); }
void ba_jacobi_scale(const BaProblem* P, const gsfm_ba_options& o) {
  hipLaunchKernelGGL(k_pos_scale, ba_grid(P->n_nodes), dim3(256), 0, P->mem.s, (uint32_t)P->n_nodes, P->Dg, P->S, o.jacobi_scaling);
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

// PCG on Sc y_c = rhs from y_c = 0 (k_ba_pcg_init set r, z, p, q): lm_loop.hpp's driver, with the breakdown rule
int ba_pcg(gsfm_ba_problem* P, const gsfm_ba_options& o, BaStep* out) {
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams;
  V.dot(P->r, P->z, nullptr, N, BS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + BS_RZA, P->scal + BS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    ba_schur_product(P, P->q, P->p, P->Ap);
    V.dot(P->p, P->Ap, nullptr, N, BS_PAP);
    hipLaunchKernelGGL(k_pos_pcg_update, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, BS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, N, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, ba_grid(N), dim3(256), 0, P->mem.s, N, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, true, iterate, V.pcg_reader(), &out->cg, &out->stalled, &out->cg_rel);
}

// One LM step's linear algebra at P->x, after its linearisation and with the Jacobi scale in place -- shared by the solve and by
// gsfm_ba_step_check.  Leaves y (cameras, then points), delta, the trial point P->cand and scal[BS_STEP2], [BS_DG], [BS_DLD] enqueued.
int ba_step(gsfm_ba_problem* P, double radius, const gsfm_ba_options& o, BaStep* out) {
  const uint32_t N = P->n_cams, T = P->n_tracks;
  const size_t NN = P->n_nodes;
  const DevScalars V = P->vec();
  *out = BaStep();
  ba_prep(P, radius, o);
  // reduced right-hand side b_c - E~ C~^-1 b_p (zt holds -S C~^-1 b_p), the Schur-Jacobi preconditioner, the PCG start
  hipLaunchKernelGGL(k_ba_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)nullptr, (const double*)P->zt, (const double*)nullptr,
                     (const double*)P->S, (const double*)P->D2, (const double*)P->b, P->rhs, 0);
  hipLaunchKernelGGL(k_ba_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Cfix, P->Minv);
  hipLaunchKernelGGL(k_ba_pcg_init, ba_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->rhs, P->Minv, P->S, P->y, P->r, P->z, P->p, P->q);
  if (int st = ba_pcg(P, o, out)) return st;
  // back-substitution y_p = C~^-1 (b_p - E~^T y_c), with q = S y_c
  hipLaunchKernelGGL(k_ba_scale, ba_grid(N), dim3(256), 0, P->mem.s, (size_t)N, P->active, P->S, P->y, 1.0, P->q);
  if (T > 0) BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)P->b, P->y + 3 * (size_t)N, 0);
  // the step, its gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_ba_scale, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->S, P->y, -1.0, P->delta);
  if (o.remove_gauge && P->n_active > 0) {
    for (int c = 0; c < 3; ++c) {
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)P->delta, P->active, NN, c, P->part);
      V.reduce(BS_SUMD + c);
      hipLaunchKernelGGL(k_ba_axis_sum, dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, (const double*)P->x, P->active, NN, c, P->part);
      V.reduce(BS_SUMX + c);
    }
    hipLaunchKernelGGL(k_ba_center, ba_grid(NN), dim3(256), 0, P->mem.s, NN, P->active, P->scal, (int)BS_SUMD, (int)BS_SUMX, 1.0 / (double)P->n_active, P->x, P->delta, P->v);
  } else {
    HIPCHK(hipMemsetAsync(P->v, 0, 24 * NN, P->mem.s));
  }
  V.dot(P->delta, P->v, nullptr, NN, BS_DV);
  V.dot(P->v, P->v, nullptr, NN, BS_VV);
  hipLaunchKernelGGL(k_pos_project, ba_grid(NN), dim3(256), 0, P->mem.s, (uint32_t)NN, P->scal, BS_DV, BS_VV, P->v, P->delta, P->x, P->cand);
  V.dot(P->delta, P->delta, nullptr, NN, BS_STEP2);
  V.dot(P->delta, P->g, nullptr, NN, BS_DG);
  BA_TRACKS(P, k_ba_quad_tracks, (const double*)P->delta, P->pt_scratch);
  ba_sum(P, P->pt_scratch, T, BS_DLD);
  return 0;
}

// What lm_loop runs for either bundle adjustment.  hs: the host copy of the device scalars up to BS_N.
struct BaLm {
  BaProblem* P;
  const gsfm_ba_options& o;
  gsfm_ba_summary* sum;
  double hs[BS_N];
  int read_scal(const char* what) { return P->vec().read(hs, P->scal, sizeof(hs), what); }
  int start(LmPoint* at) {
    P->cost(P->x, nullptr, nullptr);
    P->linearize();
    ba_jacobi_scale(P, o);
    ba_norms(P);
    if (int st = read_scal("start point")) return st;
    *at = {hs[BS_COST], hs[BS_GMAX], hs[BS_XNORM2]};
    return 0;
  }
  int step(double radius, LmStep* out) {
    BaStep step;
    if (int st = P->step(radius, o, &step)) return st;
    sum->num_cg_iterations += step.cg;
    if (step.stalled) sum->num_pcg_stalled_steps++;
    if (int st = read_scal("step")) return st;
    *out = {hs[BS_STEP2], hs[BS_DG], hs[BS_DLD], step.cg};
    return 0;
  }
  int trial_cost(double* cost) {
    P->cost(P->cand, nullptr, nullptr);
    return P->vec().read_slot(BS_COST, cost, "trial cost");
  }
  int accept(LmPoint* at) {
    HIPCHK(hipMemcpyAsync(P->x, P->cand, 24 * P->n_nodes, hipMemcpyDeviceToDevice, P->mem.s));
    P->linearize();
    ba_norms(P);
    if (int st = read_scal("linearisation")) return st;
    at->gmax = hs[BS_GMAX]; at->xnorm2 = hs[BS_XNORM2];
    return 0;
  }
};

gsfm_ba_options ba_options(const gsfm_ba_options* opt, void (*defaults)(gsfm_ba_options*) = gsfm_ba_options_default) {
  gsfm_ba_options o;
  if (opt) return *opt;
  defaults(&o);
  return o;
}

// x = (cam_pos, points), enqueued
int ba_upload_point(gsfm_ba_problem* P, const double* cam_pos, const double* points) {
  if (P->n_cams) HIPCHK(hipMemcpyAsync(P->x, cam_pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->mem.s));
  if (P->n_tracks) HIPCHK(hipMemcpyAsync(P->x + 3 * (size_t)P->n_cams, points, 24 * (size_t)P->n_tracks, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}
// what a solve does before its first step, after the upload of x: cost and linearisation there, the Jacobi scale of that point
int ba_setup_linearize(BaProblem* P, const gsfm_ba_options& o, double* cost) {
  P->cost(P->x, nullptr, nullptr);
  P->linearize();
  ba_jacobi_scale(P, o);
  if (int st = P->vec().read_slot(BS_COST, cost, "linearisation")) return st;
  P->have_lin = true;
  return 0;
}
bool ba_needs_points(const gsfm_ba_problem* P, const double* cam_pos, const double* points) {
  return (P->n_cams > 0 && !cam_pos) || (P->n_tracks > 0 && !points);
}

// ---- problem creation ----
// The checks of the track arrays (track_scene.hpp), on the host before any device call.  nodes_per_cam: 1, or 2 or 3 for the full bundle adjustment.
int ba_check_tracks(uint32_t n_cams, int nodes_per_cam, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy,
                    const char* entry) {
  if (int st = track_arrays_check(n_cams, n_tracks, track_ptr, obs_cam, obs_xy, TrackLimit::observations_and_nodes, (uint64_t)nodes_per_cam * n_cams,
                                  "NULL argument (track_ptr holds n_tracks + 1 entries)")) return st;
  if (const char* why = no_device_reason(entry)) return fail(GSFM_ERR_NO_DEVICE, why);
  return 0;
}

// The host side of a new problem: sizes, the host structure, the active byte of every node (a camera's nodes_per_cam nodes carry the
// camera's), the lane classes (order: n_tracks entries, uploaded by ba_upload_structure) and the NULL loss
void ba_init(BaProblem* P, uint32_t n_cams, int nodes_per_cam, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
             const uint32_t* obs_cam, const uint8_t* point_estimated, uint32_t* order) {
  const size_t N = n_cams, T = n_tracks;
  (void)hipGetDevice(&P->device);
  P->n_cams = n_cams; P->n_tracks = (uint32_t)n_tracks; P->n_obs = track_ptr[n_tracks]; P->n_nodes = nodes_per_cam * N + T;
  P->st = ba_build_structure(n_cams, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated);
  P->n_used = P->st.n_used;
  P->n_active = (uint64_t)P->st.n_active_cams + P->st.n_active_points;
  P->h_active.resize(P->n_nodes);
  for (int k = 0; k < nodes_per_cam; ++k) std::copy(P->st.cam_active.begin(), P->st.cam_active.end(), P->h_active.begin() + k * N);
  std::copy(P->st.point_active.begin(), P->st.point_active.end(), P->h_active.begin() + nodes_per_cam * N);
  tri_bucket(T, track_ptr, order, P->cb);
  std::memset(&P->leaf, 0, sizeof(P->leaf));
  P->leaf.kind = GSFM_LOSS_TRIVIAL;
}

inline hipError_t ba_up(hipStream_t s, void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; }

// The slab: committed, placed (place: ba_place / fba_place), its zeroed part cleared, the structure arrays uploaded
template <typename Pb, typename Place>
int ba_commit_upload(Pb* P, Place place, const char* who, const uint64_t* track_ptr, const uint32_t* order, const uint32_t* obs_cam, const double* obs_xy,
                     size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs;
  if (int st = P->mem.commit(place(P, nullptr, zeroed), who, 0)) return st;
  place(P, P->mem.slab, zeroed);
  const hipStream_t s = P->mem.s;
  HIPCHK(hipMemsetAsync(P->mem.slab, 0, *zeroed, s));
  HIPCHK(ba_up(s, P->track_ptr, track_ptr, 8 * (T + 1))); HIPCHK(ba_up(s, P->order, order, 4 * T));
  HIPCHK(ba_up(s, P->obs_cam, obs_cam, 4 * O)); HIPCHK(ba_up(s, P->obs_xy, obs_xy, 16 * O));
  HIPCHK(ba_up(s, P->crow_ptr, P->st.row_ptr.data(), 4 * (N + 1))); HIPCHK(ba_up(s, P->cobs, P->st.obs.data(), 4 * P->n_used)); HIPCHK(ba_up(s, P->ctrk, P->st.trk.data(), 4 * P->n_used));
  HIPCHK(ba_up(s, P->track_used, P->st.track_used.data(), T)); HIPCHK(ba_up(s, P->active, P->h_active.data(), P->n_nodes));
  return 0;
}

// The arrays of the slab in order.  *zeroed: the bytes one memset clears.
FlatLayout ba_place(gsfm_ba_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, T = P->n_tracks, O = P->n_obs, U = P->n_used, NN = P->n_nodes;
  SlabTake take{FlatLayout(), slab};
  take(P->scal, BS_N); take(P->Dg, 6 * NN);
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->y, &P->delta, &P->v}) take(*v, 3 * NN);
  for (double** v : {&P->rhs, &P->r, &P->z, &P->p, &P->q, &P->Ap}) take(*v, 3 * N);
  take(P->zt, 3 * T); take(P->pt_scratch, T); take(P->Cfix, GSFM_BA_FIX_DOUBLES * T);   // (no point is flagged before the first k_ba_prep_points)
  *zeroed = take.L.total;
  take(P->Minv, 9 * N); take(P->Cinv, 9 * T); take(P->Gt, 6 * T); take(P->part, GSFM_POS_PARTS);
  take(P->cams, GSFM_TRI_CAM_DOUBLES * N); take(P->Ht, 6 * O); take(P->At, 3 * O); take(P->Hc, 6 * U);
  take(P->obs_xy, O); take(P->track_ptr, T + 1);
  take(P->order, T); take(P->obs_cam, O); take(P->crow_ptr, N + 1); take(P->cobs, U); take(P->ctrk, U);
  take(P->track_used, T); take(P->active, NN);
  return take.L;
}

gsfm_status ba_create_impl(uint32_t n_cams, const double* rot_aa, const double* intrinsics, const uint8_t* cam_estimated, uint64_t n_tracks,
                           const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated, gsfm_ba_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (n_cams > 0 && (!rot_aa || !intrinsics)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = ba_check_tracks(n_cams, 1, n_tracks, track_ptr, obs_cam, obs_xy, "gsfm_ba_problem_create")) return (gsfm_status)st;
  const size_t N = n_cams;
  hvec<uint32_t> order(n_tracks);
  // upload staging that must outlive the enqueued copies: declared before P (whose destroy waits for the stream)
  std::vector<uint8_t> est(N, 1);
  if (cam_estimated) for (size_t k = 0; k < N; ++k) est[k] = cam_estimated[k] != 0;
  std::unique_ptr<gsfm_ba_problem, void (*)(gsfm_ba_problem*)> P(new gsfm_ba_problem, gsfm_ba_problem_destroy);
  ba_init(P.get(), n_cams, 1, cam_estimated, n_tracks, track_ptr, obs_cam, point_estimated, order.data());
  size_t zeroed = 0;
  if (int st = ba_commit_upload(P.get(), ba_place, "the bundle adjustment problem", track_ptr, order.data(), obs_cam, obs_xy, &zeroed)) return (gsfm_status)st;
  const hipStream_t s = P->mem.s;
  // the camera records from rot_aa and f u v (positions are unknowns: the record's position field stays zero); staged in cand / g / D2, x still zero
  if (N > 0) {
    HIPCHK_S(ba_up(s, P->cand, rot_aa, 24 * N)); HIPCHK_S(ba_up(s, P->g, intrinsics, 24 * N));
    HIPCHK_S(ba_up(s, P->D2, est.data(), N));
    hipLaunchKernelGGL(k_tri_cameras, ba_grid(N), dim3(256), 0, s, n_cams, (const double*)P->cand, (const double*)P->x, (const double*)P->g, (const uint8_t*)P->D2, P->cams);
    HIPCHK_S(hipMemsetAsync(P->mem.slab, 0, zeroed, s));
  }
  if (int st = sync_stream(s, "bundle adjustment problem create")) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
}

// A solve around what differs: upload() enqueues x = the caller's point, scatter(xh) copies the active rows of the result to the caller's
// arrays (only the active nodes are parameters: every other row keeps its bytes).  tag: the solver's name in the verbose line.
template <typename Upload, typename Scatter>
gsfm_status ba_solve(BaProblem* P, const gsfm_ba_options& o, gsfm_ba_summary* summary, const char* tag, Upload upload, Scatter scatter) {
  gsfm_ba_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->num_observations_used = P->n_used; summary->num_active_cameras = P->st.n_active_cams; summary->num_active_points = P->st.n_active_points;
  summary->termination = GSFM_TERM_GRADIENT_TOLERANCE;
  if (P->n_used == 0) return GSFM_OK;   // nothing to adjust: nothing changes
  const double t0 = now_ms();
  if (int st = upload()) return (gsfm_status)st;
  BaLm ops{P, o, summary, {}};
  if (int st = lm_loop(ops, o, summary, tag)) return (gsfm_status)st;
  hvec<double> xh(3 * P->n_nodes);
  if (int st = P->vec().read(xh.data(), P->x, 24 * P->n_nodes, "download the estimates")) return (gsfm_status)st;
  scatter(xh.data());
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status ba_solve_impl(gsfm_ba_problem* P, double* cam_pos, double* points, const gsfm_ba_options* opt, gsfm_ba_summary* summary) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks;
  return ba_solve(P, ba_options(opt), summary, "ba", [&] { return ba_upload_point(P, cam_pos, points); }, [&](const double* xh) {
    for (size_t k = 0; k < N; ++k) if (P->h_active[k]) std::copy(&xh[3 * k], &xh[3 * k] + 3, cam_pos + 3 * k);
    for (size_t t = 0; t < T; ++t) if (P->h_active[N + t]) std::copy(&xh[3 * (N + t)], &xh[3 * (N + t)] + 3, points + 3 * t);
  });
}

gsfm_status ba_linearize_impl(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* cost, double* grad_cam, double* grad_point,
                              double* diag_cam, double* diag_point) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams, T = P->n_tracks, NN = N + T;
  double c = 0.0;
  if (int st = ba_upload_point(P, cam_pos, points)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, ba_options(nullptr), &c)) return (gsfm_status)st;
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

// Residuals and rho of every observation at the caller's point (upload() enqueues it into x), through a scratch buffer of the call
template <typename Upload>
gsfm_status ba_residuals(BaProblem* P, Upload upload, double* r_out, double* rho_out) {
  const size_t O = P->n_obs;
  if (O == 0) return GSFM_OK;
  FlatLayout L;
  const Slot<double> r = L.take<double>(2 * O), rho = L.take<double>(O);
  DevBuf<char> scratch;
  if (scratch.alloc(L.total) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  if (int st = upload()) return (gsfm_status)st;
  P->cost(P->x, (double*)(scratch.p + r.off), (double*)(scratch.p + rho.off));
  if (r_out) HIPCHK_S(hipMemcpyAsync(r_out, scratch.p + r.off, 16 * O, hipMemcpyDeviceToHost, P->mem.s));
  if (rho_out) HIPCHK_S(hipMemcpyAsync(rho_out, scratch.p + rho.off, 8 * O, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "residuals");
}

gsfm_status ba_residuals_impl(gsfm_ba_problem* P, const double* cam_pos, const double* points, double* r_out, double* rho_out) {
  if (!P || ba_needs_points(P, cam_pos, points)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  return ba_residuals(P, [&] { return ba_upload_point(P, cam_pos, points); }, r_out, rho_out);
}

// set_loss of either bundle adjustment (who: its name in the messages); nothing is read of P before the last refusal
gsfm_status ba_set_loss(BaProblem* P, const gsfm_loss_node* prog, int32_t n, const char* who) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  gsfm::DevLossNode leaf;
  if (int st = one_leaf_loss(prog, n, who, &leaf)) return (gsfm_status)st;
  P->leaf = leaf;   // (passed to the kernels by value)
  P->have_lin = false;
  return GSFM_OK;
}

// Device time of single launches for the *_time_kernels entries: timer(launch) runs launch once to warm, then reps times between two events,
// and appends the mean in microseconds to out_us; after a failure (st) it does nothing
struct KernelTimer {
  hipStream_t s;
  int reps;
  double* out_us;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int st = 0, k = 0;
  int create() { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); return 0; }
  ~KernelTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  template <typename Launch> void operator()(Launch launch) {
    if (st) return;
    launch();   // warm
    (void)hipEventRecord(e0, s);
    for (int r = 0; r < reps; ++r) launch();
    (void)hipEventRecord(e1, s);
    st = sync_stream(s, "time_kernels");
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    out_us[k++] = 1e3 * ms / reps;
  }
};

}  // namespace

void gsfm_ba_problem::cost(const double* at, double* r_out, double* rho_out) { ba_cost(this, at, r_out, rho_out); }
void gsfm_ba_problem::linearize() { ba_linearize(this); }
int gsfm_ba_problem::step(double radius, const gsfm_ba_options& o, BaStep* out) { return ba_step(this, radius, o, out); }

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
  gsfm_ba_options o = ba_options(nullptr);
  double cost = 0.0;
  if (int st = ba_upload_point(P, cam_pos, points)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
  BaStep step;
  o.max_cg_iterations = 1;   // one step's setup (D^2, the points' inverses, q, p) is all the timed kernels need
  if (int st = ba_step(P, radius, o, &step)) return (gsfm_status)st;
  KernelTimer timed{P->mem.s, reps, out_us};
  if (int st = timed.create()) return (gsfm_status)st;
  const uint32_t N = P->n_cams;
  timed([&] { BA_TRACKS(P, k_ba_lin_tracks, (const double*)P->x, P->g, P->Dg); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_lin, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), P->g, P->Dg); });
  timed([&] { BA_TRACKS(P, k_ba_cost_tracks, (const double*)P->x, P->pt_scratch, (double*)nullptr, (double*)nullptr); });
  timed([&] { BA_TRACKS(P, k_ba_point_pass, (const double*)P->q, (const double*)P->S, (const double*)P->Cinv, (const double*)P->Cfix, (const double*)nullptr, P->zt, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_pass, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->q, (const double*)P->zt, (const double*)P->p,
                                 (const double*)P->S, (const double*)P->D2, (const double*)nullptr, P->Ap, 1); });
  timed([&] { hipLaunchKernelGGL(k_ba_cam_precond, ba_row_grid(N), dim3(256), 0, P->mem.s, ba_dev(P), (const double*)P->S, (const double*)P->D2, (const double*)P->Gt, (const double*)P->Cinv, (const double*)P->Cfix, P->Minv); });
  return (gsfm_status)timed.st;
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

gsfm_status gsfm_ba_set_loss(gsfm_ba_problem* P, const gsfm_loss_node* prog, int32_t n) { return ba_set_loss(P, prog, n, "bundle adjustment"); }

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
  ba_jacobi_scale(P, o);
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
  if (int st = ba_upload_point(P, cam_pos, points)) return (gsfm_status)st;
  if (int st = ba_setup_linearize(P, o, &cost)) return (gsfm_status)st;
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
