// Host side of camera-position estimation (include/gsfm_pos.h): problem assembly, the operations that lm_loop.hpp's Levenberg-Marquardt loop
// and PCG driver run (PosLm, pos_pcg), exact steps by the dense tiled Cholesky (solver_dense.hpp, enqueue_chol_solve) or block-Jacobi PCG.  The
// kernels are in pos_kernels.hpp; the host sequences launches and reads a few scalars per LM iteration (and one per cg_check_interval PCG
// iterations).
// Memory: every array a problem always has lies in one slab laid out by FlatLayout and owned, with the problem's private non-blocking
// stream, by a FlatCall member (flat_call.hpp).  The dense tiles and the callback buffers are allocated on first use.  Every copy and
// memset in this file is ordered on that stream (host_common.hpp, DevBuf: the transfer rule), the loss tables of a MAGSAC leaf included.
#pragma once
#include "host_common.hpp"
#include "flat_call.hpp"
#include "pos_structure.hpp"
#include "lm_loop.hpp"
#include "dev_scalars.hpp"
#include "solver_launch.hpp"
#include "solver_dense.hpp"
#include "pos_kernels.hpp"
#include "../../include/gsfm_pos.h"

#include <memory>

struct gsfm_pos_problem {
  int device = 0;
  FlatCall mem;                            // the stream (mem.s) and the slab of the arrays below that are plain pointers (pos_place)
  uint32_t n_cams = 0;
  uint64_t n_edges = 0;
  std::vector<uint8_t> present, h_active;  // camera appears in an edge; staging of the active set (pos_upload_point)
  uint32_t *row_ptr = nullptr, *nbr = nullptr, *eid = nullptr, *ei = nullptr, *ej = nullptr;
  double *dir_k = nullptr, *dir_e = nullptr, *H = nullptr;
  uint8_t* active = nullptr;
  // per camera (3 or more doubles each)
  double *x = nullptr, *cand = nullptr, *g = nullptr, *Dg = nullptr, *S = nullptr, *D2 = nullptr, *Mblk = nullptr, *Minv = nullptr, *b = nullptr, *r = nullptr,
         *z = nullptr, *p = nullptr, *q = nullptr, *y = nullptr, *Ap = nullptr, *delta = nullptr, *v = nullptr, *part = nullptr, *scal = nullptr;
  DevBuf<double> denseA, denseL, dense_x;  // (first exact step)
  DevBuf<int> dense_info;
  // loss
  DevLoss* d_loss = nullptr;
  DevBuf<double> tables[3];
  int lm = LM_SIMPLE;                      // kernel specialisation of the in-kernel loss (LM_SIMPLE / LM_PROGRAM); unused under a callback loss
  gsfm_loss_callback cb = nullptr;
  void* cb_user = nullptr;
  DevBuf<double> rho_ext, s_dev;           // (first callback loss)
  std::vector<double> h_s, h_rho;
  bool have_lin = false;                   // a linearisation from gsfm_pos_linearize / gsfm_pos_step_check is on the device
  DevScalars vec() const { return {mem.s, part, scal}; }
};

namespace {

using gsfm::PosDev;

enum { PS_RZ0 = PCG_RZ0, PS_RZA = PCG_RZA, PS_RZB = PCG_RZB, PS_PAP = 3, PS_DV = 4, PS_VV = 5, PS_STEP2 = 6, PS_DG = 7, PS_DLD = 8, PS_COST = 9, PS_GMAX = 10,
       PS_XNORM2 = 11, PS_N = 12 };
static_assert(LM_TERM_FUNCTION_TOLERANCE == GSFM_TERM_FUNCTION_TOLERANCE && LM_TERM_GRADIENT_TOLERANCE == GSFM_TERM_GRADIENT_TOLERANCE &&
              LM_TERM_PARAMETER_TOLERANCE == GSFM_TERM_PARAMETER_TOLERANCE && LM_TERM_NO_CONVERGENCE == GSFM_TERM_NO_CONVERGENCE &&
              LM_TERM_FAILURE == GSFM_TERM_FAILURE, "lm_loop.hpp restates the termination codes");

PosDev pos_dev(gsfm_pos_problem* P) {
  PosDev a{};
  a.n_cams = P->n_cams; a.n_edges = (uint32_t)P->n_edges;
  a.row_ptr = P->row_ptr; a.nbr = P->nbr; a.eid = P->eid; a.dir_k = P->dir_k; a.ei = P->ei; a.ej = P->ej; a.dir_e = P->dir_e;
  a.active = P->active; a.H = P->H; a.loss = P->d_loss; a.rho_ext = P->rho_ext.p;
  return a;
}
inline dim3 pos_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline dim3 pos_row_grid(uint32_t n_cams) { return dim3((n_cams + 3) / 4); }

// The kernel specialisations of the problem's loss: an in-kernel leaf or program, or (linearisation only: a callback's cost is summed on
// the host, pos_callback_rho) the rho triples the host supplied per edge.
auto pos_cost_kernel(const gsfm_pos_problem* P) { return P->lm == LM_SIMPLE ? k_pos_cost<LM_SIMPLE> : k_pos_cost<LM_PROGRAM>; }
auto pos_lin_kernel(const gsfm_pos_problem* P) {
  if (P->cb) return k_pos_lin<POS_LM_EXT>;
  return P->lm == LM_SIMPLE ? k_pos_lin<LM_SIMPLE> : k_pos_lin<LM_PROGRAM>;
}

// host-callback loss: s of every edge at pos, rho from the callback (in edge order), the triples uploaded for the linearisation; returns the cost
int pos_callback_rho(gsfm_pos_problem* P, const double* pos, double* cost) {
  hipLaunchKernelGGL(k_pos_resid, pos_grid(P->n_edges), dim3(256), 0, P->mem.s, pos_dev(P), pos, (double*)nullptr, P->s_dev.p, (double*)nullptr, 0);
  if (int st = P->vec().read(P->h_s.data(), P->s_dev.p, 8 * P->n_edges, "callback residuals")) return st;
  double c = 0.0;
  for (size_t e = 0; e < P->n_edges; ++e) { P->cb(P->cb_user, P->h_s[e], &P->h_rho[3 * e]); c += 0.5 * P->h_rho[3 * e]; }
  *cost = c;
  return 0;
}

// cost of pos into scal[PS_COST] (in-kernel loss) or *cost (callback: then also the rho triples at pos are staged in h_rho)
int pos_cost(gsfm_pos_problem* P, const double* pos, double* cost) {
  if (P->cb) return pos_callback_rho(P, pos, cost);
  hipLaunchKernelGGL(pos_cost_kernel(P), dim3(GSFM_POS_PARTS), dim3(256), 0, P->mem.s, pos_dev(P), pos, P->part);
  P->vec().reduce(PS_COST);
  return 0;
}

// linearisation at P->x (the callback's rho triples of x must be in h_rho)
int pos_linearize(gsfm_pos_problem* P) {
  if (P->cb) HIPCHK(hipMemcpyAsync(P->rho_ext.p, P->h_rho.data(), 24 * P->n_edges, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(pos_lin_kernel(P), pos_row_grid(P->n_cams), dim3(256), 0, P->mem.s, pos_dev(P), P->x, P->g, P->Dg);
  return P->cb ? sync_stream(P->mem.s, "linearisation") : 0;   // (h_rho is overwritten by the next trial point)
}

// What every solve, linearisation and step check starts with: the cost of P->x (*cb_cost under a callback loss, else scal[PS_COST]) and
// the linearisation there.
int pos_start(gsfm_pos_problem* P, double* cb_cost) {
  if (int st = pos_cost(P, P->x, cb_cost)) return st;
  return pos_linearize(P);
}

// gradient max norm and |x| over the free parameters into scal[PS_GMAX], scal[PS_XNORM2]
void pos_norms(gsfm_pos_problem* P) { P->vec().norms(P->g, P->x, P->active, P->n_cams, PS_GMAX, PS_XNORM2); }

// Exact step by the dense tiled Cholesky; *ok = false: not used (size, memory; *info = -1) or the factorisation met a non-positive pivot
// (*info > 0).  K_tiles (may be NULL): a host copy of the assembled tiles, taken before the factorisation overwrites them.
int pos_dense_step(gsfm_pos_problem* P, bool* ok, int* info_out, std::vector<double>* K_tiles) {
  *ok = false; *info_out = -1;
  const uint32_t n = 3 * P->n_cams, T = (n + GSFM_CB - 1) / GSFM_CB;
  if (T > GSFM_DENSE_MAX_T) return 0;
  const size_t elems = chol_num_tiles(T) * GSFM_TILE_ELEMS;
  if (!P->denseA.p) {
    if (P->denseA.alloc(elems) != hipSuccess || P->denseL.alloc_zeroed(elems, P->mem.s) != hipSuccess ||
        P->dense_x.alloc_zeroed((size_t)T * GSFM_CB, P->mem.s) != hipSuccess ||
        P->dense_info.alloc(1) != hipSuccess) {
      P->denseA.release(); P->denseL.release(); P->dense_x.release(); (void)hipGetLastError();
      return 0;
    }
  }
  HIPCHK(hipMemsetAsync(P->denseA.p, 0, 8 * elems, P->mem.s));
  HIPCHK(hipMemsetAsync(P->dense_info.p, 0, sizeof(int), P->mem.s));
  hipLaunchKernelGGL(k_pos_dense_assemble, dim3(P->n_cams), dim3(256), 0, P->mem.s, pos_dev(P), P->S, P->Mblk, P->b, P->denseA.p, n, T);
  if (K_tiles) {
    K_tiles->resize(elems);
    if (int st = P->vec().read(K_tiles->data(), P->denseA.p, 8 * elems, "dense assembly")) return st;
  }
  enqueue_chol_solve(P->denseA.p, P->denseL.p, P->dense_x.p, n, T, P->dense_info.p, P->mem.s, false);
  HIPCHK(hipMemcpyAsync(P->y, P->dense_x.p, 8 * (size_t)n, hipMemcpyDeviceToDevice, P->mem.s));
  int info = 0;
  if (int st = P->vec().read(&info, P->dense_info.p, sizeof(int), "dense step")) return st;
  *info_out = info;
  *ok = info == 0;
  return 0;
}

// PCG on (S L S + D^2) y = b from y = 0 (k_pos_prep set r, z, p, q): lm_loop.hpp's driver, without the breakdown rule
int pos_pcg(gsfm_pos_problem* P, const gsfm_pos_options& o, int* iters, bool* stalled, double* rel) {
  const PosDev a = pos_dev(P);
  const DevScalars V = P->vec();
  const uint32_t N = P->n_cams;
  V.dot(P->r, P->z, nullptr, N, PS_RZ0);
  HIPCHK(hipMemcpyAsync(P->scal + PS_RZA, P->scal + PS_RZ0, 8, hipMemcpyDeviceToDevice, P->mem.s));
  auto iterate = [&](int cur, int nxt) {
    hipLaunchKernelGGL(k_pos_matvec<true>, pos_row_grid(N), dim3(256), 0, P->mem.s, a, P->q, P->p, P->S, P->D2, P->Ap);
    V.dot(P->p, P->Ap, nullptr, N, PS_PAP);
    hipLaunchKernelGGL(k_pos_pcg_update, pos_grid(N), dim3(256), 0, P->mem.s, N, P->scal, cur, PS_PAP, P->p, P->Ap, P->y, P->r, P->z, P->Minv);
    V.dot(P->r, P->z, nullptr, N, nxt);
    hipLaunchKernelGGL(k_pos_pcg_dir, pos_grid(N), dim3(256), 0, P->mem.s, N, P->scal, nxt, cur, P->active, P->S, P->z, P->p, P->q);
  };
  return pcg_loop(o, false, iterate, V.pcg_reader(), iters, stalled, rel);
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
  const DevScalars V = P->vec();
  *out = PosStep();
  auto prep = [&] {
    hipLaunchKernelGGL(k_pos_prep, pos_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->Dg, P->g, P->S, radius, o.min_lm_diagonal, o.max_lm_diagonal,
                       P->D2, P->Mblk, P->Minv, P->b, P->r, P->z, P->p, P->q, P->y);
  };
  prep();
  bool solved = false;
  if ((int64_t)N <= (int64_t)o.dense_max_cams) {
    if (int st = pos_dense_step(P, &solved, &out->info, K_tiles)) return st;
    if (!solved) prep();
  }
  out->dense = solved;
  if (!solved)
    if (int st = pos_pcg(P, o, &out->cg, &out->stalled, &out->cg_rel)) return st;
  // the step, its scale-gauge part removed, the trial point, and what the decision needs
  hipLaunchKernelGGL(k_pos_step, pos_grid(N), dim3(256), 0, P->mem.s, N, P->active, P->S, P->y, P->x, fixed, o.remove_scale_gauge, P->delta, P->v);
  V.dot(P->delta, P->v, nullptr, N, PS_DV);
  V.dot(P->v, P->v, nullptr, N, PS_VV);
  hipLaunchKernelGGL(k_pos_project, pos_grid(N), dim3(256), 0, P->mem.s, N, P->scal, PS_DV, PS_VV, P->v, P->delta, P->x, P->cand);
  V.dot(P->delta, P->delta, nullptr, N, PS_STEP2);
  V.dot(P->delta, P->g, nullptr, N, PS_DG);
  hipLaunchKernelGGL(k_pos_matvec<false>, pos_row_grid(N), dim3(256), 0, P->mem.s, a, P->delta, P->delta, P->S, P->D2, P->Ap);
  V.dot(P->delta, P->Ap, nullptr, N, PS_DLD);
  return 0;
}

// What lm_loop runs for the position problem.  hs: the host copy of the device scalars.
struct PosLm {
  gsfm_pos_problem* P;
  int32_t fixed;
  const gsfm_pos_options& o;
  gsfm_pos_summary* sum;
  double hs[PS_N];
  int read_scal(const char* what) { return P->vec().read(hs, P->scal, sizeof(hs), what); }
  int start(LmPoint* at) {
    const uint32_t N = P->n_cams;
    double cb_cost = 0.0;
    if (int st = pos_start(P, &cb_cost)) return st;
    hipLaunchKernelGGL(k_pos_scale, pos_grid(N), dim3(256), 0, P->mem.s, N, P->Dg, P->S, o.jacobi_scaling);
    pos_norms(P);
    if (int st = read_scal("start point")) return st;
    *at = {P->cb ? cb_cost : hs[PS_COST], hs[PS_GMAX], hs[PS_XNORM2]};
    return 0;
  }
  int step(double radius, LmStep* out) {
    PosStep step;
    if (int st = pos_step(P, fixed, radius, o, &step, nullptr)) return st;
    if (step.dense) sum->num_dense_solves++;
    else {
      sum->num_cg_iterations += step.cg;
      if (step.stalled) sum->num_pcg_stalled_steps++;
    }
    if (int st = read_scal("step")) return st;
    *out = {hs[PS_STEP2], hs[PS_DG], hs[PS_DLD], step.cg};
    return 0;
  }
  int trial_cost(double* cost) {
    if (int st = pos_cost(P, P->cand, cost)) return st;
    return P->cb ? 0 : P->vec().read_slot(PS_COST, cost, "trial cost");
  }
  int accept(LmPoint* at) {
    HIPCHK(hipMemcpyAsync(P->x, P->cand, 24 * (size_t)P->n_cams, hipMemcpyDeviceToDevice, P->mem.s));
    if (int st = pos_linearize(P)) return st;
    pos_norms(P);
    if (int st = read_scal("linearisation")) return st;
    at->gmax = hs[PS_GMAX]; at->xnorm2 = hs[PS_XNORM2];
    return 0;
  }
};

// fixed_cam is -1 or a camera that appears in an edge
int pos_check_fixed(const gsfm_pos_problem* P, int32_t fixed_cam) {
  if (fixed_cam >= -1 && fixed_cam < (int64_t)P->n_cams && (fixed_cam < 0 || P->present[fixed_cam])) return 0;
  return fail(GSFM_ERR_INVALID_ARG, "fixed_cam must be -1 or a camera that appears in an edge");
}
gsfm_pos_options pos_options(const gsfm_pos_options* opt) {
  gsfm_pos_options o;
  if (opt) return *opt;
  gsfm_pos_options_default(&o);
  return o;
}

// The active set (the present cameras, less fixed_cam when >= 0) and x = pos, enqueued
int pos_upload_point(gsfm_pos_problem* P, const double* pos, int32_t fixed_cam) {
  P->h_active = P->present;
  if (fixed_cam >= 0) P->h_active[fixed_cam] = 0;
  HIPCHK(hipMemcpyAsync(P->active, P->h_active.data(), P->h_active.size(), hipMemcpyHostToDevice, P->mem.s));
  HIPCHK(hipMemcpyAsync(P->x, pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->mem.s));
  return 0;
}

// ... and the cost and the linearisation at x: what a solve does before its first step.  *cost: the cost of pos.
int pos_setup_linearize(gsfm_pos_problem* P, const double* pos, int32_t fixed_cam, double* cost) {
  if (int st = pos_upload_point(P, pos, fixed_cam)) return st;
  if (int st = pos_start(P, cost)) return st;
  if (!P->cb) HIPCHK(hipMemcpyAsync(cost, P->scal + PS_COST, 8, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearisation")) return st;
  P->have_lin = true;
  return 0;
}

// ---- problem creation: argument checks, the host structure (pos_structure.hpp), layout and commit, upload and k_pos_directions ----
int pos_check_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa) {
  if (n_cams == 0 || n_edges == 0) return fail(GSFM_ERR_EMPTY, "no cameras or no edges");
  if (!edge_i || !edge_j || !rel_t || !rot_aa) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31) || n_cams >= (1u << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges or cameras)");
  for (uint64_t e = 0; e < n_edges; ++e)
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams || edge_i[e] == edge_j[e]) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has a bad camera index");
  if (const char* why = no_device_reason("gsfm_pos_problem_create")) return fail(GSFM_ERR_NO_DEVICE, why);
  return 0;
}

// The arrays of the slab in order: laid out (slab == NULL), then pointed into the committed slab.  Those a new problem finds zeroed come
// first, side by side (*zeroed bytes): one memset clears them.
FlatLayout pos_place(gsfm_pos_problem* P, char* slab, size_t* zeroed) {
  const size_t N = P->n_cams, E = P->n_edges, ND = 2 * E;
  SlabTake take{FlatLayout(), slab};
  take(P->active, N); take(P->scal, PS_N); take(P->Dg, 6 * N);
  take(P->d_loss, 1);   // (all zeros: Ceres' NULL loss, the default; the estimator layer sets the reference's HuberLoss(0.1))
  for (double** v : {&P->x, &P->cand, &P->g, &P->S, &P->D2, &P->b, &P->r, &P->z, &P->p, &P->q, &P->y, &P->Ap, &P->delta, &P->v}) take(*v, 3 * N);
  *zeroed = take.L.total;
  take(P->row_ptr, N + 1); take(P->nbr, ND); take(P->eid, ND); take(P->ei, E); take(P->ej, E);
  take(P->dir_k, 3 * ND); take(P->dir_e, 3 * E); take(P->H, 6 * ND);
  take(P->Mblk, 6 * N); take(P->Minv, 9 * N); take(P->part, GSFM_POS_PARTS);
  return take.L;
}

// k_pos_directions' inputs that the problem does not keep: one allocation of create's, gone when it returns
struct PosTmp {
  FlatLayout L;
  Slot<uint32_t> pos_i, pos_j;
  Slot<double> rel, rot;
  DevBuf<char> buf;
  PosTmp(size_t N, size_t E) : pos_i(L.take<uint32_t>(E)), pos_j(L.take<uint32_t>(E)), rel(L.take<double>(3 * E)), rot(L.take<double>(3 * N)) {}
  template <typename T> T* ptr(Slot<T> h) const { return (T*)(buf.p + h.off); }
};

// tmp is allocated first, so that the slab's memory check (FlatCall::commit, on the exact total) sees what is left beside it
int pos_layout_commit(gsfm_pos_problem* P, PosTmp& tmp) {
  if (tmp.buf.alloc(tmp.L.total) != hipSuccess) { (void)hipGetLastError(); return fail(GSFM_ERR_HIP, "allocating the upload buffers of the position problem failed"); }
  size_t zeroed = 0;
  if (int st = P->mem.commit(pos_place(P, nullptr, &zeroed), "the position problem", 0)) return st;
  pos_place(P, P->mem.slab, &zeroed);
  HIPCHK(hipMemsetAsync(P->mem.slab, 0, zeroed, P->mem.s));
  return 0;
}

int pos_upload(gsfm_pos_problem* P, const PosStructure& S, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
               const PosTmp& tmp) {
  const size_t N = P->n_cams, E = P->n_edges;
  auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, P->mem.s); };
  HIPCHK(up(P->row_ptr, S.row_ptr.data(), 4 * (N + 1))); HIPCHK(up(P->nbr, S.nbr.data(), 8 * E)); HIPCHK(up(P->eid, S.eid.data(), 8 * E));
  HIPCHK(up(P->ei, edge_i, 4 * E)); HIPCHK(up(P->ej, edge_j, 4 * E));
  HIPCHK(up(tmp.ptr(tmp.pos_i), S.pos_i.data(), 4 * E)); HIPCHK(up(tmp.ptr(tmp.pos_j), S.pos_j.data(), 4 * E));
  HIPCHK(up(tmp.ptr(tmp.rel), rel_t, 24 * E)); HIPCHK(up(tmp.ptr(tmp.rot), rot_aa, 24 * N));
  hipLaunchKernelGGL(k_pos_directions, pos_grid(E), dim3(256), 0, P->mem.s, (uint32_t)E, P->ei, (const double*)tmp.ptr(tmp.rot), (const double*)tmp.ptr(tmp.rel),
                     (const uint32_t*)tmp.ptr(tmp.pos_i), (const uint32_t*)tmp.ptr(tmp.pos_j), P->dir_e, P->dir_k);
  return sync_stream(P->mem.s, "position problem create");
}

gsfm_status pos_create_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t, const double* rot_aa,
                            gsfm_pos_problem** out) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL output pointer");
  *out = nullptr;
  if (int st = pos_check_create(n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa)) return (gsfm_status)st;
  PosStructure S = pos_build_structure(n_cams, n_edges, edge_i, edge_j);
  PosTmp tmp(n_cams, n_edges);
  // (declared behind S and tmp: on a failure gsfm_pos_problem_destroy waits for the stream while what the enqueued copies read and write is alive)
  std::unique_ptr<gsfm_pos_problem, void (*)(gsfm_pos_problem*)> P(new gsfm_pos_problem, gsfm_pos_problem_destroy);
  (void)hipGetDevice(&P->device);
  P->n_cams = n_cams; P->n_edges = n_edges;
  P->present.swap(S.present);
  if (int st = pos_layout_commit(P.get(), tmp)) return (gsfm_status)st;
  if (int st = pos_upload(P.get(), S, edge_i, edge_j, rel_t, rot_aa, tmp)) return (gsfm_status)st;
  *out = P.release();
  return GSFM_OK;
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
  if (P->mem.s) (void)hipStreamSynchronize(P->mem.s);
  delete P;
}

gsfm_status gsfm_pos_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                    const double* rot_aa, gsfm_pos_problem** out) {
  return guarded("position problem creation", pos_create_impl, n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa, out);
}

gsfm_status gsfm_pos_set_loss(gsfm_pos_problem* P, const gsfm_loss_node* prog, int32_t n) {
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
  P->cb = nullptr;
  HIPCHK_S(hipMemcpyAsync(P->d_loss, &L, sizeof(L), hipMemcpyHostToDevice, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "set_loss");
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
  if (int st = pos_check_fixed(P, fixed_cam)) return (gsfm_status)st;
  DeviceGuard g(P->device);
  const gsfm_pos_options o = pos_options(opt);
  gsfm_pos_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  summary->num_edges_used = P->n_edges;
  const double t0 = now_ms();
  if (int st = pos_upload_point(P, pos, fixed_cam)) return (gsfm_status)st;
  PosLm ops{P, fixed_cam, o, summary, {}};
  if (int st = lm_loop(ops, o, summary, "pos")) return (gsfm_status)st;
  HIPCHK_S(hipMemcpyAsync(pos, P->x, 24 * (size_t)P->n_cams, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "download positions")) return (gsfm_status)st;
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status gsfm_pos_residuals(gsfm_pos_problem* P, const double* pos, double* r_out, double* rho_out) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t E = P->n_edges;
  FlatLayout L;
  const Slot<double> r = L.take<double>(3 * E), rho = L.take<double>(E), s_slot = L.take<double>(E);
  DevBuf<char> scratch;
  if (scratch.alloc(L.total) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc residual buffers");
  double *d_r = (double*)(scratch.p + r.off), *d_rho = (double*)(scratch.p + rho.off), *d_s = (double*)(scratch.p + s_slot.off);
  HIPCHK_S(hipMemcpyAsync(P->cand, pos, 24 * (size_t)P->n_cams, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_pos_resid, pos_grid(E), dim3(256), 0, P->mem.s, pos_dev(P), P->cand, d_r, d_s, d_rho, P->cb ? 0 : 1);
  std::vector<double> s(E);
  if (r_out) HIPCHK_S(hipMemcpyAsync(r_out, d_r, 24 * E, hipMemcpyDeviceToHost, P->mem.s));
  if (rho_out && !P->cb) HIPCHK_S(hipMemcpyAsync(rho_out, d_rho, 8 * E, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(s.data(), d_s, 8 * E, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "residuals")) return (gsfm_status)st;
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
  HIPCHK_S(hipMemcpyAsync(g3.data(), P->g, 24 * N, hipMemcpyDeviceToHost, P->mem.s));
  HIPCHK_S(hipMemcpyAsync(d6.data(), P->Dg, 48 * N, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "linearize outputs")) return (gsfm_status)st;
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
  HIPCHK_S(hipMemcpyAsync(P->q, v, 24 * N, hipMemcpyHostToDevice, P->mem.s));
  hipLaunchKernelGGL(k_pos_matvec<false>, pos_row_grid(P->n_cams), dim3(256), 0, P->mem.s, pos_dev(P), P->q, P->q, P->S, P->D2, P->Ap);
  HIPCHK_S(hipMemcpyAsync(y, P->Ap, 24 * N, hipMemcpyDeviceToHost, P->mem.s));
  return (gsfm_status)sync_stream(P->mem.s, "normal_matvec");
}

gsfm_status gsfm_pos_step_check(gsfm_pos_problem* P, const double* pos, int32_t fixed_cam, double radius, const gsfm_pos_options* opt, double* K_out,
                                double* b_out, double* y_out, double* delta_out, double* scal_out, int32_t* info_out) {
  if (!P || !pos) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = pos_check_fixed(P, fixed_cam)) return (gsfm_status)st;
  if (!(radius > 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive");
  DeviceGuard g(P->device);
  const gsfm_pos_options o = pos_options(opt);
  const uint32_t N = P->n_cams, n = 3 * N;
  double cost = 0.0;
  if (int st = pos_setup_linearize(P, pos, fixed_cam, &cost)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_pos_scale, pos_grid(N), dim3(256), 0, P->mem.s, N, P->Dg, P->S, o.jacobi_scaling);
  PosStep step;
  std::vector<double> tiles;
  if (int st = pos_step(P, fixed_cam, radius, o, &step, K_out ? &tiles : nullptr)) return (gsfm_status)st;
  double hs[PS_N];
  HIPCHK_S(hipMemcpyAsync(hs, P->scal, sizeof(hs), hipMemcpyDeviceToHost, P->mem.s));
  if (b_out) HIPCHK_S(hipMemcpyAsync(b_out, P->b, 8 * (size_t)n, hipMemcpyDeviceToHost, P->mem.s));
  if (y_out) HIPCHK_S(hipMemcpyAsync(y_out, P->y, 8 * (size_t)n, hipMemcpyDeviceToHost, P->mem.s));
  if (delta_out) HIPCHK_S(hipMemcpyAsync(delta_out, P->delta, 8 * (size_t)n, hipMemcpyDeviceToHost, P->mem.s));
  if (int st = sync_stream(P->mem.s, "step check")) return (gsfm_status)st;
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
