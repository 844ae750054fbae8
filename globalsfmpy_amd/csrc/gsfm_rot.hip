// C-ABI implementation (include/gsfm_rot.h): problem assembly, Levenberg-Marquardt control with
// Ceres 1.14 trust-region semantics, block-Jacobi PCG orchestration.  All arithmetic on the edges
// and cameras runs in the kernels of kernels.hpp; the host only sequences launches and reads a
// handful of scalars per LM iteration.  The one-shot calls (host arrays in, host arrays out) are
// one line each here: their bodies are the *_impl functions of the headers below, all on the
// scratch owner of flat_call.hpp.  Built with hipcc --offload-arch=gfx950 into libgsfm_rot.so.
#include "host_common.hpp"
#include "solver_launch.hpp"
#include "solver_pcg.hpp"
#include "solver_dense.hpp"
#include "solver_components.hpp"
#include "solver_lm.hpp"
#include "problem_create.hpp"
#include "edge_norms.hpp"
#include "spanning_tree.hpp"
#include "dense_check.hpp"
#include "cov_estimate.hpp"
#include "solver_pos.hpp"
#include "trans_filter.hpp"
#include "trans_refine.hpp"
#include "triangulate.hpp"
#include "track_refine.hpp"
#include "outlier_tracks.hpp"
#include "track_build.hpp"
#include "track_select.hpp"
#include "solver_ba.hpp"
#include "solver_full_ba.hpp"
#include "solver_pos_points.hpp"
#include "rot_l1l2.hpp"

// =============================================================================================
extern "C" {

int gsfm_rot_abi_version(void) { return GSFM_ROT_ABI_VERSION; }
const char* gsfm_last_error(void) { return g_err.c_str(); }

void gsfm_rot_options_default(gsfm_rot_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 200; o->num_threads = 1;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
  o->jacobi_scaling = 1; o->max_cg_iterations = 20000; o->cg_relative_tolerance = 1e-12; o->cg_check_interval = 8; o->verbose = 0; o->pcg_single_reduction = -1; o->cg_stall_iterations = 0; o->dense_cholesky_max_cams = 512; o->pcg_hip_graph = 1;
  o->pcg_forcing = 1; o->pcg_forcing_tolerance = 1e-8; o->dense_cholesky_auto_cams = 5333; o->lm_device_control = 1; o->component_rest = 1;
}

int32_t gsfm_rot_residual_dim(int32_t t) { return t == GSFM_ROT_QUATERNION_NORM ? 4 : t == GSFM_ROT_ROTATION_MAT_FNORM ? 9 : 3; }

gsfm_status gsfm_rot_problem_create(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, int32_t error_type,
                                    const double* cov6, const double* inlier_weight, const gsfm_rot_shard* shard, gsfm_rot_problem** out) {
  // The host-side structure build allocates O(E) vectors and starts threads: an exception (std::bad_alloc, std::system_error) must not
  // cross the C boundary.  (On a sharded problem the peers of a rank that fails THIS way are not told: they wait in the agreement.)
  gsfm_rot_problem* live = nullptr;
  try {
    return problem_create_impl(n_cams, n_edges, edge_i, edge_j, rel_aa, error_type, cov6, inlier_weight, shard, out, &live);
  } catch (const std::exception& e) {
    if (live) gsfm_rot_problem_destroy(live);
    if (out) *out = nullptr;
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, std::string("problem creation ran out of host resources: ") + e.what());
  }
}

void gsfm_rot_problem_destroy(gsfm_rot_problem* P) {
  if (!P) return;
  DeviceGuard g(P->device);
  P->timer.destroy();
  P->reset_pcg_graphs();
  if (P->dense_graph) (void)hipGraphExecDestroy(P->dense_graph);
  P->comps.drop_graph(); P->comps.drop_side();
  if (P->own_stream && P->stream) (void)hipStreamDestroy(P->stream);
  if (P->pin) (void)hipHostFree(P->pin);
  if (P->rec_host) (void)hipHostFree(P->rec_host);
  if (P->mail_host) (void)hipHostFree(P->mail_host);
  delete P;
}

gsfm_status gsfm_rot_set_stream(gsfm_rot_problem* P, void* s) {
  if (!P) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL problem");
  DeviceGuard g(P->device);
  if (P->stream) (void)hipStreamSynchronize(P->stream);   // (whatever the problem enqueued on the stream it leaves, a loss upload say, has arrived)
  if (P->own_stream && P->stream) (void)hipStreamDestroy(P->stream);
  P->reset_pcg_graphs(); P->pcg_graph.unusable = false; P->pcg2_graph.unusable = false;
  if (P->dense_graph) { (void)hipGraphExecDestroy(P->dense_graph); P->dense_graph = nullptr; }
  P->comps.drop_graph(); P->comps.drop_side();
  if (s) { P->stream = (hipStream_t)s; P->own_stream = false; }
  else { if (hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "hipStreamCreate failed"); P->own_stream = true; }
  P->timer.stream = P->stream;
  return GSFM_OK;
}

gsfm_status gsfm_rot_set_loss(gsfm_rot_problem* P, const gsfm_loss_node* prog, int32_t n) {
  if (!P || (n > 0 && !prog)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  P->cb = nullptr;
  return (gsfm_status)prepare_loss(P, prog, n);
}

gsfm_status gsfm_rot_set_loss_callback(gsfm_rot_problem* P, gsfm_loss_callback fn, void* user) {
  if (!P || !fn) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  if (!P->rho_ext.p) {
    if (P->rho_ext.alloc(3 * P->n_edges_in) != hipSuccess || P->s_ext.alloc(P->n_edges_in) != hipSuccess)
      return (gsfm_status)fail(GSFM_ERR_HIP, "allocating callback-loss buffers failed");
  }
  P->cb = fn; P->cb_user = user;
  return GSFM_OK;
}

gsfm_status gsfm_rot_set_edge_weights(gsfm_rot_problem* P, const double* w) {
  if (!P || !w) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (P->functor != F_AA || P->wmode == W_MATRIX) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge weights only apply to the scalar-weight angle-axis types");
  DeviceGuard g(P->device);
  if (int st = promote_to_scalar_weights(P)) return (gsfm_status)st;
  if (!P->w_orig.p && P->w_orig.alloc(P->n_edges_in) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc weights");
  if (hipMemcpyAsync(P->w_orig.p, w, 8 * P->n_edges_in, hipMemcpyHostToDevice, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "upload weights");
  if (P->cost.n) hipLaunchKernelGGL(k_gather_weights, dim3(grid_for(P->cost.n)), dim3(GSFM_BLOCK), 0, P->stream, P->w_orig.p, P->cost.eid.p, P->cost.n, P->cost.ws.p);
  if (P->dir.n) hipLaunchKernelGGL(k_gather_weights, dim3(grid_for(P->dir.n)), dim3(GSFM_BLOCK), 0, P->stream, P->w_orig.p, P->dir.eid.p, P->dir.n, P->dir.ws.p);
  return (gsfm_status)sync_check(P, "set_edge_weights");
}

static gsfm_status solve_impl(gsfm_rot_problem* P, double* rot, const gsfm_rot_options* opt, gsfm_rot_summary* summary, bool resident);
gsfm_status gsfm_rot_solve(gsfm_rot_problem* P, double* rot, const gsfm_rot_options* opt, gsfm_rot_summary* summary) { return solve_impl(P, rot, opt, summary, false); }
// rot: DEVICE memory on the problem's device, caller numbering, 3 doubles per camera, in / out.  Returns with the problem's stream synchronised.
gsfm_status gsfm_rot_solve_resident(gsfm_rot_problem* P, double* rot_dev, const gsfm_rot_options* opt, gsfm_rot_summary* summary) {
  if (P && rot_dev) {
    DeviceGuard g(P->device);
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, rot_dev) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
      (void)hipGetLastError();
      return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "gsfm_rot_solve_resident: rot_aa_dev_inout is not device memory (host arrays go to gsfm_rot_solve)");
    }
  }
  return solve_impl(P, rot_dev, opt, summary, true);
}
static gsfm_status solve_impl(gsfm_rot_problem* P, double* rot, const gsfm_rot_options* opt, gsfm_rot_summary* summary, bool resident) {
  if (!P || !rot) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const gsfm_rot_options o = opt ? *opt : default_options();
  gsfm_rot_summary local; if (!summary) summary = &local;
  const double t0 = now_ms();
  if (int st = upload_state(P, rot, resident)) return (gsfm_status)st;
  int st = lm_solve(P, o, summary);
  if (st == GSFM_INTERNAL_RESTART) {
    // The forcing schedule gave up on this trajectory after inexact steps had been applied (solver_lm.hpp, the contraction gate): the solve is
    // redone from the caller's rotations -- still untouched in `rot` -- with every step exact; what the abandoned attempt spent stays on the bill.
    const gsfm_rot_summary spent = *summary;
    gsfm_rot_options o2 = o;
    o2.pcg_forcing = 0;
    if (o.verbose) fprintf(stderr, "[gsfm] forcing schedule abandoned after %d LM iterations (steps stopped contracting): restarting with exact steps\n", spent.num_iterations);
    if (int st2 = upload_state(P, rot, resident)) return (gsfm_status)st2;
    st = lm_solve(P, o2, summary);
    summary->num_forcing_restarts = 1;
    add_work(summary, spent);
  }
  if (st) return (gsfm_status)st;
  if (int st2 = resident ? download_state_resident(P, rot) : download_state(P, rot)) return (gsfm_status)st2;
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

// EstimateRotationsWithSigmaConsensus (estimator.cpp:314-457)
gsfm_status gsfm_rot_solve_sigma_consensus(gsfm_rot_problem* P, double* rot, int32_t iters_num, double sigma_max,
                                           const gsfm_rot_options* opt, gsfm_rot_summary* summary) {
  if (!P || !rot) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (P->error_type != GSFM_ROT_ANGLE_AXIS) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "sigma consensus needs an ANGLE_AXIS problem");
  DeviceGuard g(P->device);
  const gsfm_rot_options o = opt ? *opt : default_options();
  gsfm_rot_summary local, total; if (!summary) summary = &local;
  std::memset(&total, 0, sizeof(total));
  const double t0 = now_ms();
  // The scalar-weight planes live on the device for the whole loop, each in its kernel's own order.  There is no weight pass: the first
  // cost sweep and the first linearisation of every inner solve start from exactly the rotations the reference computes the weights at
  // (:378-416), so they compute, store and use them (setup_kernels.hpp, SigmaDev).  The first comparison is against zero weights, like the
  // reference's zero-initialised last_weights (:352-353).
  if (int st = promote_to_scalar_weights(P)) return (gsfm_status)st;
  if (P->cost.n) HIPCHK_S(hipMemsetAsync(P->cost.ws.p, 0, 8 * P->cost.n, P->stream));
  if (int st = ensure_sigma(P, sigma_max, &P->sigma)) return (gsfm_status)st;
  double global_edges = (double)P->n_edges_in;
  if (P->sharded) {
    // every edge is counted in mean |w - w_old| by exactly one rank: its cost owner
    const double mine = (double)P->cost.n;
    HIPCHK_S(hipMemcpyAsync(P->sigma_sum.p + 1, &mine, 8, hipMemcpyHostToDevice, P->stream));
    if (int st = all_reduce(P, P->sigma_sum.p + 1, 1)) return (gsfm_status)st;
    HIPCHK_S(hipMemcpyAsync(&global_edges, P->sigma_sum.p + 1, 8, hipMemcpyDeviceToHost, P->stream));
    if (int st = sync_check(P, "sigma consensus: edge count")) return (gsfm_status)st;
  }
  int outer = 0;
  for (int it = 0; it < iters_num; ++it) {
    ++outer;
    P->sigma_pending_cost = P->sigma_pending_lin = true;   // consumed by the solve's first K1 / K2
    const gsfm_status sst = gsfm_rot_solve(P, rot, &o, summary);
    P->sigma_pending_cost = P->sigma_pending_lin = false;
    if (sst) return sst;
    // sum |w - w_old| was left on the device by that first sweep: read it now, after the solve (the decision it feeds comes after the
    // solve in the reference too, :448)
    if (int st = all_reduce(P, P->sigma_sum.p, 1)) return (gsfm_status)st;
    double avg = 0.0;
    if (hipMemcpyAsync(&avg, P->sigma_sum.p, 8, hipMemcpyDeviceToHost, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "read weight change");
    if (int st = sync_check(P, "sigma consensus weights")) return (gsfm_status)st;
    avg /= global_edges;
    if (it == 0) total = *summary;
    else {
      add_work(&total, *summary);
      total.num_iterations += summary->num_iterations; total.num_successful_steps += summary->num_successful_steps;
      total.num_unsuccessful_steps += summary->num_unsuccessful_steps; total.num_dense_solves += summary->num_dense_solves;
      total.final_cost = summary->final_cost; total.termination = summary->termination;
      total.final_gradient_max_norm = summary->final_gradient_max_norm; total.final_radius = summary->final_radius;
      total.num_forcing_refinements += summary->num_forcing_refinements; total.num_inexact_steps += summary->num_inexact_steps;
      total.num_pcg_capped_steps += summary->num_pcg_capped_steps; total.num_forcing_restarts += summary->num_forcing_restarts;
      total.worst_accepted_cg_residual = std::fmax(total.worst_accepted_cg_residual, summary->worst_accepted_cg_residual);
    }
    total.last_weight_change = avg;
    if (avg <= 1e-7) break;  // :448
  }
  total.outer_iterations = outer; total.t_total_ms = now_ms() - t0;
  *summary = total;
  return GSFM_OK;
}

gsfm_status gsfm_rot_residuals(gsfm_rot_problem* P, const double* rot, double* s_out, double* rho_out, double* r_out, double* cost) {
  if (!P || !rot) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t E = P->n_edges_in, Ec = P->cost.n, R = (size_t)P->res_dim;
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  // The sweep writes in the problem's own edge order (coalesced); the caller's order is restored here, at the C-ABI edge, on the host:
  // out[edge_order[u]] = device[u].  Edges this rank does not count in the cost (sharded problems) stay zero.
  DevBuf<double> dr; DevBuf<double2> dsr, dr12;
  if (((s_out || rho_out) && dsr.alloc(Ec) != hipSuccess) || (rho_out && dr12.alloc(Ec) != hipSuccess) || (r_out && dr.alloc(R * Ec) != hipSuccess))
    return (gsfm_status)fail(GSFM_ERR_HIP, "alloc outputs");
  CostOutputs out;
  out.srho = dsr.p; out.rho12 = dr12.p; out.r = dr.p;
  if (int st = launch_cost(P, P->q.p, SC_COST, out)) return (gsfm_status)st;
  double h[SC_N];
  if (int st = read_scalars(P, h)) return (gsfm_status)st;
  if (cost) *cost = h[SC_COST];
  const std::vector<uint32_t>& ord = P->h_cost_eid;
  std::vector<double> stage;
  if (s_out || rho_out) {   // device planes: (s, rho) and (rho', rho'') per edge
    stage.resize(4 * Ec);
    if (Ec) if (int st = read_back(P, stage.data(), dsr.p, 16 * Ec, "copy s / rho")) return (gsfm_status)st;
    if (Ec && rho_out) if (int st = read_back(P, stage.data() + 2 * Ec, dr12.p, 16 * Ec, "copy rho', rho''")) return (gsfm_status)st;
    if (s_out) { std::memset(s_out, 0, 8 * E); for (size_t u = 0; u < Ec; ++u) s_out[ord[u]] = stage[2 * u]; }
    if (rho_out) {
      std::memset(rho_out, 0, 24 * E);
      for (size_t u = 0; u < Ec; ++u) { double* o = rho_out + 3 * (size_t)ord[u]; o[0] = stage[2 * u + 1]; o[1] = stage[2 * Ec + 2 * u]; o[2] = stage[2 * Ec + 2 * u + 1]; }
    }
  }
  if (r_out) {
    stage.resize(R * Ec);
    if (Ec) if (int st = read_back(P, stage.data(), dr.p, 8 * R * Ec, "copy r")) return (gsfm_status)st;
    std::memset(r_out, 0, 8 * R * E);
    for (size_t u = 0; u < Ec; ++u) for (size_t k = 0; k < R; ++k) r_out[R * (size_t)ord[u] + k] = stage[k * Ec + u];
  }
  return GSFM_OK;
}

int64_t gsfm_rot_edge_order(gsfm_rot_problem* P, uint32_t* order_out, uint64_t cap) {
  if (!P) { fail(GSFM_ERR_INVALID_ARG, "NULL problem"); return -1; }
  const size_t n = P->h_cost_eid.size();
  if (order_out) std::memcpy(order_out, P->h_cost_eid.data(), 4 * std::min<size_t>(n, cap));
  return (int64_t)n;
}

gsfm_status gsfm_rot_linearize(gsfm_rot_problem* P, const double* rot, double* gradient, double* diag_blocks, double* cost) {
  if (!P || !rot) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams;
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  if (int st = launch_cost(P, P->q.p, SC_COST)) return (gsfm_status)st;
  if (int st = launch_lin(P, P->q.p)) return (gsfm_status)st;
  DevBuf<double> dg, dblk;
  if (dg.alloc(3 * N) != hipSuccess || dblk.alloc(9 * N) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc outputs");
  hipLaunchKernelGGL(k_cam_export, dim3(grid_for(N)), dim3(GSFM_BLOCK), 0, P->stream, P->x.p, P->gD.p, P->n_cams, P->param_dim, dg.p, dblk.p, P->D6.p);
  double h[SC_N];
  if (int st = read_scalars(P, h)) return (gsfm_status)st;
  if (cost) *cost = h[SC_COST];
  std::vector<double> stage;
  if (!P->perm.empty()) stage.resize(9 * N);
  if (gradient) {
    if (int st = read_back(P, P->perm.empty() ? gradient : stage.data(), dg.p, 24 * N, "copy gradient")) return (gsfm_status)st;
    if (!P->perm.empty()) to_external(P, stage.data(), gradient, 3);
  }
  if (diag_blocks) {
    if (int st = read_back(P, P->perm.empty() ? diag_blocks : stage.data(), dblk.p, 72 * N, "copy blocks")) return (gsfm_status)st;
    if (!P->perm.empty()) to_external(P, stage.data(), diag_blocks, 9);
  }
  return GSFM_OK;
}

gsfm_status gsfm_rot_normal_matvec(gsfm_rot_problem* P, const double* v, double* y) {
  if (!P || !v || !y) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!P->have_lin) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "call gsfm_rot_linearize first");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams;
  // y = T^T B_eta (T v): xcg <- v, p <- T v, Ap <- B p, xcg <- T^T Ap
  if (hipMemcpyAsync(P->xcg.p, to_internal(P, v, 3), 24 * N, hipMemcpyHostToDevice, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "upload v");
  hipLaunchKernelGGL(k_cam_apply_T, dim3(grid_for(N)), dim3(GSFM_BLOCK), 0, P->stream, P->x.p, P->n_cams, P->param_dim, 0, P->xcg.p, P->p.p);
  if (P->lin_is_lap) hipLaunchKernelGGL(k_cam_rotT, dim3(grid_for(N)), dim3(GSFM_BLOCK), 0, P->stream, (const double*)P->p.p, P->q_lin, P->n_cams, P->u_rot.p);
  if (int st = launch_matvec(P, P->D6.p, P->p.p, P->Ap.p, nullptr)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_cam_apply_T, dim3(grid_for(N)), dim3(GSFM_BLOCK), 0, P->stream, P->x.p, P->n_cams, P->param_dim, 1, P->Ap.p, P->xcg.p);
  double* dst = y;
  if (!P->perm.empty()) { P->h_cam.resize(3 * N); dst = P->h_cam.data(); }
  if (hipMemcpyAsync(dst, P->xcg.p, 24 * N, hipMemcpyDeviceToHost, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "download y");
  if (int st = sync_check(P, "normal_matvec")) return (gsfm_status)st;
  if (!P->perm.empty()) to_external(P, dst, y, 3);
  return GSFM_OK;
}

gsfm_status gsfm_rot_loss_eval(gsfm_rot_problem* P, const double* s, uint64_t n, double* rho3_out, double* value_out, double* rho1_fast_out) {
  if (!P || (n > 0 && !s)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (P->cb) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "loss_eval needs a native loss program (a host-callback loss runs on the host)");
  if (n == 0) return GSFM_OK;
  DeviceGuard g(P->device);
  DevBuf<double> ds, d3, dv, d1;
  const int lm = loss_mode(P);
  if (rho1_fast_out && lm == LM_PROGRAM) { for (uint64_t k = 0; k < n; ++k) rho1_fast_out[k] = std::numeric_limits<double>::quiet_NaN(); rho1_fast_out = nullptr; }   // K2 has no fast path for this program
  if (ds.alloc(n) != hipSuccess || (rho3_out && d3.alloc(3 * n) != hipSuccess) || (value_out && dv.alloc(n) != hipSuccess) || (rho1_fast_out && d1.alloc(n) != hipSuccess)) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc");
  HIPCHK_S(hipMemcpyAsync(ds.p, s, 8 * n, hipMemcpyHostToDevice, P->stream));
  const dim3 grid(grid_for(n)), blk(GSFM_BLOCK);
  switch (lm) {   // the specialisation K1 / K2 are dispatched on for this program
    case LM_SIMPLE: hipLaunchKernelGGL(k_loss_eval<LM_SIMPLE>, grid, blk, 0, P->stream, (const DevLoss*)P->d_loss.p, (const double*)ds.p, (size_t)n, d3.p, dv.p, d1.p); break;
    case LM_MAGSAC: hipLaunchKernelGGL(k_loss_eval<LM_MAGSAC>, grid, blk, 0, P->stream, (const DevLoss*)P->d_loss.p, (const double*)ds.p, (size_t)n, d3.p, dv.p, d1.p); break;
    default: hipLaunchKernelGGL(k_loss_eval<LM_PROGRAM>, grid, blk, 0, P->stream, (const DevLoss*)P->d_loss.p, (const double*)ds.p, (size_t)n, d3.p, dv.p, d1.p); break;
  }
  if (rho1_fast_out) HIPCHK_S(hipMemcpyAsync(rho1_fast_out, d1.p, 8 * n, hipMemcpyDeviceToHost, P->stream));
  if (rho3_out) HIPCHK_S(hipMemcpyAsync(rho3_out, d3.p, 24 * n, hipMemcpyDeviceToHost, P->stream));
  if (value_out) HIPCHK_S(hipMemcpyAsync(value_out, dv.p, 8 * n, hipMemcpyDeviceToHost, P->stream));
  return (gsfm_status)sync_check(P, "loss_eval");
}

gsfm_status gsfm_rot_edge_sq_norms(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                                   const double* cov6, const double* rot_aa, double max_sq_norm, double* s_out, uint8_t* keep_out,
                                   uint64_t* n_kept, double* kernel_ms) {
  return guarded("the edge sweep", edge_sq_norms_impl, n_cams, n_edges, edge_i, edge_j, rel_aa, cov6, rot_aa, max_sq_norm, s_out, keep_out, n_kept,
                 kernel_ms);
}

gsfm_status gsfm_rot_init_spanning_tree(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                                        const int32_t* weight, double* rot_aa_out, int64_t* parent_edge_out, uint32_t* root_out,
                                        uint32_t* n_tree_cams_out, uint32_t* depth_out, double* kernel_ms) {
  return guarded("spanning-tree initialisation", init_spanning_tree_impl, n_cams, n_edges, edge_i, edge_j, rel_aa, weight, rot_aa_out,
                 parent_edge_out, root_out, n_tree_cams_out, depth_out, kernel_ms);
}

gsfm_status gsfm_pos_filter_relative_translations(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_t,
                                                  const double* rot_aa, int32_t n_axes, const double* axes, uint64_t seed, double tolerance,
                                                  double* bad_weight_out, uint8_t* keep_out, uint64_t* n_kept, double* stats_out, double* axes_out,
                                                  double* proj_out, uint32_t* num_passes_out, uint32_t* num_picks_out, double* kernel_ms) {
  return guarded("the translation filter", trans_filter_impl, n_cams, n_edges, edge_i, edge_j, rel_t, rot_aa, n_axes, axes, seed, tolerance,
                 bad_weight_out, keep_out, n_kept, stats_out, axes_out, proj_out, num_passes_out, num_picks_out, kernel_ms);
}

gsfm_status gsfm_pos_refine_relative_translations(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j,
                                                  const uint64_t* match_ptr, const double* matches, const double* intrinsics,
                                                  const double* rot_aa, const double* rel_t_in, double* rel_t_out, int32_t* status_out,
                                                  int32_t* iters_out, double* cost_out, double* kernel_ms) {
  return guarded("the translation refinement", trans_refine_impl, n_cams, n_edges, edge_i, edge_j, match_ptr, matches, intrinsics, rot_aa, rel_t_in,
                 rel_t_out, status_out, iters_out, cost_out, kernel_ms);
}

gsfm_status gsfm_tracks_triangulate(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                    const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                    const double* obs_xy, double min_triangulation_angle_degrees, double max_reprojection_error_pixels,
                                    double* point_out, int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out,
                                    uint64_t* counts_out, double* kernel_ms) {
  return guarded("the track triangulation", tri_impl, n_cams, rot_aa, cam_pos, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 min_triangulation_angle_degrees, max_reprojection_error_pixels, point_out, status_out, n_views_out, mean_sq_err_out, counts_out,
                 kernel_ms, nullptr);
}

void gsfm_tracks_refine_default_options(gsfm_tracks_refine_options* o) {
  if (!o) return;
  o->refine = 1; o->max_num_iterations = 100;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8; o->min_relative_decrease = 1e-3;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e12; o->min_trust_region_radius = 1e-32;
}

gsfm_status gsfm_tracks_triangulate_refine(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                           const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                           const double* obs_xy, double min_triangulation_angle_degrees, double max_reprojection_error_pixels,
                                           const gsfm_tracks_refine_options* options, const gsfm_loss_node* loss_program, int32_t n_loss_nodes,
                                           double* point_out, int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out,
                                           int32_t* iterations_out, double* initial_cost_out, double* final_cost_out, int32_t* termination_out,
                                           uint64_t* counts_out, double* kernel_ms) {
  return guarded("the track refinement", tri_refine_impl, n_cams, rot_aa, cam_pos, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 min_triangulation_angle_degrees, max_reprojection_error_pixels, options, loss_program, n_loss_nodes, point_out, status_out,
                 n_views_out, mean_sq_err_out, iterations_out, initial_cost_out, final_cost_out, termination_out, counts_out, kernel_ms);
}

gsfm_status gsfm_tracks_outlier_tracks(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                       const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                       const double* obs_xy, const double* points, const uint8_t* point_estimated,
                                       double max_reprojection_error_pixels, double min_triangulation_angle_degrees, int32_t* status_out,
                                       int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms) {
  return guarded("the outlier rule", outlier_tracks_impl, n_cams, rot_aa, cam_pos, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 points, point_estimated, max_reprojection_error_pixels, min_triangulation_angle_degrees, status_out, n_views_out,
                 mean_sq_err_out, counts_out, kernel_ms);
}

gsfm_status gsfm_tracks_launch_order(uint64_t n_tracks, const uint64_t* track_ptr, uint32_t* order_out, uint64_t* class_begin_out) {
  return guarded("the launch order", [&] {   // (the messages' strings, stable_sort's buffer)
    if (!class_begin_out || (n_tracks > 0 && (!track_ptr || !order_out))) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
    std::string why;   // (track_ptr[0] is not looked at: only the lengths matter here)
    if (!track_ptr_ok(n_tracks, track_ptr, TrackLimit::tracks, 0, false, nullptr, &why)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, why);
    tri_bucket(n_tracks, track_ptr, order_out, class_begin_out);
    return GSFM_OK;
  });
}

void gsfm_tracks_build_default_options(gsfm_tracks_build_options* o) {
  o->min_track_length = 2; o->max_track_length = 1000; o->hash_capacity_log2 = 0;
}

gsfm_status gsfm_tracks_build(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr,
                              const double* matches, const gsfm_tracks_build_options* options, uint64_t* track_ptr_out, uint32_t* obs_view_out,
                              double* obs_xy_out, uint64_t* n_tracks, uint64_t* n_obs, uint64_t* counts_out, double* kernel_ms) {
  return guarded("the track builder", tracks_build_impl, n_views, n_edges, edge_i, edge_j, match_ptr, matches, options, track_ptr_out, obs_view_out,
                 obs_xy_out, n_tracks, n_obs, counts_out, kernel_ms);
}

gsfm_status gsfm_tracks_build_sequential(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j,
                                         const uint64_t* match_ptr, const double* matches, const gsfm_tracks_build_options* options,
                                         uint64_t* track_ptr_out, uint32_t* obs_view_out, double* obs_xy_out, uint64_t* n_tracks, uint64_t* n_obs,
                                         uint64_t* counts_out, double* kernel_ms) {
  return guarded("the sequential track builder", tracks_build_sequential_impl, n_views, n_edges, edge_i, edge_j, match_ptr, matches, options,
                 track_ptr_out, obs_view_out, obs_xy_out, n_tracks, n_obs, counts_out, kernel_ms);
}

gsfm_status gsfm_tracks_select_good(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                    const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                    const double* obs_xy, const double* points, const uint8_t* point_estimated,
                                    int32_t long_track_length_threshold, int32_t image_grid_cell_size_pixels,
                                    int32_t min_num_optimized_tracks_per_view, int32_t hash_capacity_log2, uint8_t* selected_out,
                                    int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms, double* top_up_out) {
  return guarded("the track selection", select_good_impl, n_cams, rot_aa, cam_pos, intrinsics, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 points, point_estimated, long_track_length_threshold, image_grid_cell_size_pixels, min_num_optimized_tracks_per_view,
                 hash_capacity_log2, selected_out, n_views_out, mean_sq_err_out, counts_out, kernel_ms, top_up_out);
}

gsfm_status gsfm_tracks_select_good_from_statistics(uint32_t n_cams, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                                                    const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                                    const int32_t* n_views, const double* mean_sq_err, int32_t long_track_length_threshold,
                                                    int32_t image_grid_cell_size_pixels, int32_t min_num_optimized_tracks_per_view,
                                                    uint8_t* selected_out, uint64_t* counts_out) {
  return guarded("the sequential track selection", select_good_from_statistics_impl, n_cams, cam_estimated, n_tracks, track_ptr, obs_cam, obs_xy,
                 point_estimated, n_views, mean_sq_err, long_track_length_threshold, image_grid_cell_size_pixels,
                 min_num_optimized_tracks_per_view, selected_out, counts_out);
}

int64_t gsfm_rot_count_components(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j) {
  if ((n_edges > 0 && (!edge_i || !edge_j)) || n_cams >= 0x7fffffffu) { fail(GSFM_ERR_INVALID_ARG, "bad argument"); return -1; }
  for (uint64_t e = 0; e < n_edges; ++e) if (edge_i[e] >= n_cams || edge_j[e] >= n_cams) { fail(GSFM_ERR_INVALID_ARG, "edge with an out-of-range camera index"); return -1; }
  return (int64_t)count_components(n_cams, n_edges, edge_i, edge_j);
}

int32_t gsfm_rot_locality_order(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, uint32_t* perm_out) {
  if (!perm_out || (n_edges > 0 && (!edge_i || !edge_j)) || n_cams >= 0x7fffffffu || n_edges >= 0x7fffffffull) { fail(GSFM_ERR_INVALID_ARG, "bad argument"); return -1; }
  std::vector<uint32_t> ptr((size_t)n_cams + 1, 0), adj(2 * n_edges);
  for (uint64_t e = 0; e < n_edges; ++e) {
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams || edge_i[e] == edge_j[e]) { fail(GSFM_ERR_INVALID_ARG, "edge with an out-of-range or repeated camera index"); return -1; }
    ptr[edge_i[e] + 1]++; ptr[edge_j[e] + 1]++;
  }
  for (size_t c = 0; c < n_cams; ++c) ptr[c + 1] += ptr[c];
  {
    std::vector<uint32_t> fill(ptr.begin(), ptr.end() - 1);
    for (uint64_t e = 0; e < n_edges; ++e) { adj[fill[edge_i[e]]++] = edge_j[e]; adj[fill[edge_j[e]]++] = edge_i[e] | 0x80000000u; }
  }
  std::vector<uint32_t> perm;
  const bool adopted = n_edges > 0 && reorder_for_locality(n_cams, n_edges, edge_i, edge_j, ptr, adj, &perm);
  for (uint32_t c = 0; c < n_cams; ++c) perm_out[c] = adopted ? perm[c] : c;
  return adopted ? 1 : 0;
}

int32_t gsfm_rot_get_trace(gsfm_rot_problem* P, double* out, int32_t cap_rows) {
  if (!P) return 0;
  const int rows = (int)(P->trace.size() / GSFM_ROT_TRACE_COLS);
  const int m = std::min(rows, cap_rows);
  if (out && m > 0) std::memcpy(out, P->trace.data(), sizeof(double) * GSFM_ROT_TRACE_COLS * m);
  return rows;
}

gsfm_status gsfm_rot_time_sweep(gsfm_rot_problem* P, const double* rot, int32_t reps, double* mean_ms) {
  if (!P || !rot || !mean_ms || reps <= 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "bad argument");
  if (P->cb) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "time_sweep needs a native loss");
  DeviceGuard g(P->device);
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  const CostArgs a = cost_args(P, P->q.p);
  auto sweep = [&] { return dispatch<CostArgs, CostLauncher>(P, a, P->nb_cost) ? fail(GSFM_ERR_UNSUPPORTED, "dispatch") : 0; };
  return (gsfm_status)timed(P, reps, 3, 1, "time_sweep", sweep, mean_ms);
}

gsfm_status gsfm_rot_time_sweep_variants(gsfm_rot_problem* P, const double* rot, int32_t reps, double* out_ms8) {
  if (!P || !rot || !out_ms8 || reps <= 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "bad argument");
  if (P->cb) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "time_sweep_variants needs a native loss");
  DeviceGuard g(P->device);
  const size_t Ec = P->cost.n;
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  DevBuf<double> ds; DevBuf<double2> dsr, dr12;
  if (ds.alloc_zeroed(Ec, P->stream) != hipSuccess || dsr.alloc_zeroed(Ec, P->stream) != hipSuccess || dr12.alloc_zeroed(Ec, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc outputs");
  const CostArgs base = cost_args(P, P->q.p);
  // two warm-ups, the faster of two rounds; a launch that cannot be dispatched times nothing, as before
  auto time_it = [&](auto&& launch, double* out) { return timed(P, reps, 2, 2, "time_sweep_variants", [&] { launch(); return 0; }, out); };
  int st = 0;
  for (int k = 0; k < 8; ++k) out_ms8[k] = 0.0;
  { CostArgs a = base; st = time_it([&] { dispatch<CostArgs, CostLauncher>(P, a, P->nb_cost); }, &out_ms8[0]); }                                   // trial cost: rho value only
  if (!st) { CostArgs a = base; a.srho_out = dsr.p; a.rho12_out = dr12.p; st = time_it([&] { dispatch<CostArgs, CostLauncher>(P, a, P->nb_cost); }, &out_ms8[1]); }  // s + rho triple
  if (!st) { CostArgs a = base; a.s_out = ds.p; a.s_only = 1; st = time_it([&] { dispatch<CostArgs, CostLauncher>(P, a, P->nb_cost); }, &out_ms8[2]); }   // s only (callback pass 1)
  if (!st) { CostArgs a = base; a.rho1_out = ds.p; st = time_it([&] { dispatch<CostArgs, CostLauncher>(P, a, P->nb_cost); }, &out_ms8[3]); }             // the reweight sweep of SURVEY 8(d): rho' out
  if (!st && P->functor == F_AA && P->wmode == W_SCALAR && P->cost.ws.p && P->dir.ws.p) {
    // sigma consensus: the first cost sweep / linearisation of an inner solve with the weight computation fused in (estimator.cpp:400-416),
    // against the same kernels without it.  The sweeps overwrite the problem's own weight planes: save and restore them.
    SigmaDev sg{};
    st = ensure_sigma(P, 0.02, &sg); sg.on = 1;
    DevBuf<double> keep_c, keep_d;
    if (!st && (keep_c.alloc(P->cost.n) != hipSuccess || keep_d.alloc(P->dir.n) != hipSuccess)) st = fail(GSFM_ERR_HIP, "alloc");
    if (!st) {
      (void)hipMemcpyAsync(keep_c.p, P->cost.ws.p, 8 * P->cost.n, hipMemcpyDeviceToDevice, P->stream);
      (void)hipMemcpyAsync(keep_d.p, P->dir.ws.p, 8 * P->dir.n, hipMemcpyDeviceToDevice, P->stream);
      const SigmaDev keep_sigma = P->sigma;
      P->sigma = sg;
      st = time_it([&] { P->sigma_pending_cost = true; (void)launch_cost(P, P->q.p, SC_COST); }, &out_ms8[4]);    // K1 with the weights fused in (+ the two scalar reductions)
      if (!st) st = time_it([&] { (void)launch_cost(P, P->q.p, SC_COST); }, &out_ms8[5]);                          // the same sweep without
      if (!st) st = time_it([&] { P->sigma_pending_lin = true; (void)launch_lin(P, P->q.p); }, &out_ms8[6]);       // K2 with the weights fused in
      if (!st) st = time_it([&] { (void)launch_lin(P, P->q.p); }, &out_ms8[7]);                                    // K2 without
      P->sigma = keep_sigma; P->sigma_pending_cost = P->sigma_pending_lin = false;
      (void)hipMemcpyAsync(P->cost.ws.p, keep_c.p, 8 * P->cost.n, hipMemcpyDeviceToDevice, P->stream);
      (void)hipMemcpyAsync(P->dir.ws.p, keep_d.p, 8 * P->dir.n, hipMemcpyDeviceToDevice, P->stream);
      if (int s2 = sync_check(P, "time_sweep_variants restore")) st = st ? st : s2;
    }
  }
  return (gsfm_status)st;
}

namespace {
// flag |= 1 if the n 8-byte words of a and b differ anywhere (gsfm_rot_trial_lin_check)
__global__ void __launch_bounds__(GSFM_BLOCK) k_words_differ(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b, size_t n, unsigned int* flag) {
  bool diff = false;
  for (size_t k = (size_t)blockIdx.x * GSFM_BLOCK + threadIdx.x; k < n; k += (size_t)gridDim.x * GSFM_BLOCK) diff |= a[k] != b[k];
  if (__any(diff) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
}  // namespace

gsfm_status gsfm_rot_trial_lin_check(gsfm_rot_problem* P, const double* rot, const double* rot_trial, double* cost_out, int32_t* same_out) {
  if (!P || !rot || !rot_trial || !cost_out || !same_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!trial_lin_supported(P)) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "this problem has no fused trial evaluation");
  DeviceGuard g(P->device);
  const size_t N = P->n_cams;
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  if (int st = launch_lin(P, P->q.p)) return (gsfm_status)st;
  // the linearisation at rot_aa, kept aside
  DevBuf<double2> s0, s1, s2, sq;
  DevBuf<double> sgD;
  DevBuf<unsigned int> flag;
  if (s0.alloc(P->h0.n) != hipSuccess || s1.alloc(P->h1.n) != hipSuccess || s2.alloc(P->h2.n) != hipSuccess || sq.alloc(P->q.n) != hipSuccess ||
      sgD.alloc(P->gD.n) != hipSuccess || flag.alloc_zeroed(2, P->stream) != hipSuccess) return (gsfm_status)fail(GSFM_ERR_HIP, "alloc snapshot");
  HIPCHK_S(hipMemcpyAsync(s0.p, P->h0.p, 16 * P->h0.n, hipMemcpyDeviceToDevice, P->stream));
  HIPCHK_S(hipMemcpyAsync(s1.p, P->h1.p, 16 * P->h1.n, hipMemcpyDeviceToDevice, P->stream));
  HIPCHK_S(hipMemcpyAsync(s2.p, P->h2.p, 16 * P->h2.n, hipMemcpyDeviceToDevice, P->stream));
  HIPCHK_S(hipMemcpyAsync(sq.p, P->q.p, 16 * P->q.n, hipMemcpyDeviceToDevice, P->stream));
  HIPCHK_S(hipMemcpyAsync(sgD.p, P->gD.p, 8 * P->gD.n, hipMemcpyDeviceToDevice, P->stream));
  // the trial point: x_trial / q_trial, as k_cam_step leaves them
  HIPCHK_S(hipMemcpyAsync(P->aa_io.p, to_internal(P, rot_trial, 3), 24 * N, hipMemcpyHostToDevice, P->stream));
  if (P->param_dim == 3) { HIPCHK_S(hipMemcpyAsync(P->x_trial.p, P->aa_io.p, 24 * N, hipMemcpyDeviceToDevice, P->stream)); }
  else hipLaunchKernelGGL(k_cam_cache, dim3(grid_for(N)), dim3(GSFM_BLOCK), 0, P->stream, P->aa_io.p, P->n_cams, 3, (double2*)P->x_trial.p);
  launch_cache(P, P->x_trial.p, P->q_trial.p);
  if (int st = launch_lin(P, P->q_trial.p, nullptr, true, true)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(GSFM_BLOCK), 0, P->stream, (const double*)P->cs.cost_part.p, (int)P->cs.n_wg, P->scal.p + SC_TRIAL);
  if (int st = launch_cost(P, P->q_trial.p, SC_COST)) return (gsfm_status)st;
  auto differ = [&](const void* a, const void* b, size_t bytes, int slot) {
    hipLaunchKernelGGL(k_words_differ, dim3(1024), dim3(GSFM_BLOCK), 0, P->stream, (const unsigned long long*)a, (const unsigned long long*)b, bytes / 8, flag.p + slot);
  };
  differ(s0.p, P->h0.p, 16 * P->h0.n, 1); differ(s1.p, P->h1.p, 16 * P->h1.n, 1); differ(s2.p, P->h2.p, 16 * P->h2.n, 1);
  differ(sq.p, P->q.p, 16 * P->q.n, 1); differ(sgD.p, P->gD.p, 8 * P->gD.n, 1);
  // launch_lin's own linearisation at the trial point, against the fused one
  if (int st = launch_lin(P, P->q_trial.p)) return (gsfm_status)st;
  differ(P->h0_b.p, P->h0.p, 16 * P->h0.n, 0); differ(P->h1_b.p, P->h1.p, 16 * P->h1.n, 0); differ(P->h2_b.p, P->h2.p, 16 * P->h2.n, 0);
  differ(P->gD_b.p, P->gD.p, 8 * P->gD.n, 0);
  double h[SC_N];
  if (int st = read_scalars(P, h)) return (gsfm_status)st;
  unsigned int f[2] = {1, 1};
  if (int st = read_back(P, f, flag.p, sizeof(f), "trial_lin_check flags")) return (gsfm_status)st;
  cost_out[0] = h[SC_COST]; cost_out[1] = h[SC_TRIAL];
  same_out[0] = f[0] == 0; same_out[1] = f[1] == 0;
  if (int st = launch_lin(P, P->q.p)) return (gsfm_status)st;
  return (gsfm_status)sync_check(P, "trial_lin_check");
}

gsfm_status gsfm_rot_step_check(gsfm_rot_problem* P, const double* rot, double radius, double loose_tau, const gsfm_rot_options* opt, double* eta_out,
                                double* delta_out, double* x_out, double* x_trial_out, double* lam_out, double* eta_loose_out, double* delta_loose_out,
                                gsfm_rot_step_info* info) {
  return guarded("the step check", [&]() -> gsfm_status {
  if (!P || !rot) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (!(radius > 0.0) || !(loose_tau >= 0.0)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "radius must be positive and loose_tau non-negative");
  if (P->sharded) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "step_check runs on unsharded problems");
  DeviceGuard g(P->device);
  gsfm_rot_options o = opt ? *opt : default_options();
  o.initial_trust_region_radius = radius; o.max_num_iterations = std::max(o.max_num_iterations, 1);
  o.pcg_forcing = 0; o.lm_device_control = 0;   // one host-controlled, tight step (loose_tau: LmSolve::check_step)
  const size_t N = P->n_cams, pd = (size_t)P->param_dim;
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  gsfm_rot_summary sum;
  LmSolve lm{P, o, o, &sum};
  LmSolve::StepCheck c;
  int st = lm.check_step(loose_tau, &c);
  // (whatever was enqueued has run before the buffers below are read or the problem is used again, on the error path too)
  if (int s2 = sync_check(P, "step_check")) st = st ? st : s2;
  P->timer.resolve();
  if (st) return (gsfm_status)st;
  const LmSolve::Step& s = c.s;
  const bool pcg = !s.dense_used && (!s.comp_used || !P->comps.all_dense);
  const bool single = s.comp_used ? (P->coarse_n == 0 && use_single_reduction(P, lm.o)) : s.single_reduction;
  double tol_eff = 0.0, last_rel = 0.0;
  if (pcg) {
    if (single) { Cg2Scalars h{}; if (int e = read_back(P, &h, P->cg2sc.p, sizeof(h), "step_check: PCG scalars")) return (gsfm_status)e; tol_eff = h.tol; last_rel = h.last_rel; }
    else { CgScalars h{}; if (int e = read_back(P, &h, P->cgsc.p, sizeof(h), "step_check: PCG scalars")) return (gsfm_status)e; tol_eff = h.tol; last_rel = h.last_rel; }
  }
  std::vector<double> eta(3 * N), Ti(9 * N), Lm(6 * N), xt(pd * N), xs(pd * N);
  if (int e = read_back(P, eta.data(), P->xcg.p, 24 * N, "step_check: eta")) return (gsfm_status)e;
  if (int e = read_back(P, Ti.data(), P->Tinv.p, 72 * N, "step_check: Tinv")) return (gsfm_status)e;
  if (int e = read_back(P, Lm.data(), P->Lam.p, 48 * N, "step_check: Lambda")) return (gsfm_status)e;
  if (int e = read_back(P, xt.data(), P->x_trial.p, 8 * pd * N, "step_check: x_trial")) return (gsfm_status)e;
  if (int e = read_back(P, xs.data(), P->x.p, 8 * pd * N, "step_check: x")) return (gsfm_status)e;
  // internal camera k -> the caller's numbering
  std::vector<size_t> ext(N);
  for (size_t k = 0; k < N; ++k) ext[P->perm.empty() ? k : (size_t)P->perm[k]] = k;   // ext[internal] = caller's index
  const auto put = [&](const double* src, double* dst, size_t width) {
    if (dst) for (size_t k = 0; k < N; ++k) std::memcpy(dst + ext[k] * width, src + k * width, 8 * width);
  };
  // delta = Tinv eta, as k_cam_step forms it (the same products in the same order; the host compiler may contract them into fused
  // multiply-adds where the device's did not, or the reverse: up to 3 u (|Tinv| |eta|) per component away from the device's own delta)
  const auto apply_Tinv = [&](const double* e, std::vector<double>* d) {
    d->resize(3 * N);
    for (size_t k = 0; k < N; ++k) {
      const double* T = &Ti[9 * k]; const double* v = e + 3 * k;
      for (int r = 0; r < 3; ++r) (*d)[3 * k + r] = T[3 * r] * v[0] + T[3 * r + 1] * v[1] + T[3 * r + 2] * v[2];
    }
  };
  std::vector<double> tmp;
  put(eta.data(), eta_out, 3);
  if (delta_out) { apply_Tinv(eta.data(), &tmp); put(tmp.data(), delta_out, 3); }
  put(xt.data(), x_trial_out, pd);
  put(xs.data(), x_out, pd);
  if (c.loose_cg >= 0) {
    put(c.eta_loose.data(), eta_loose_out, 3);
    if (delta_loose_out) { apply_Tinv(c.eta_loose.data(), &tmp); put(tmp.data(), delta_loose_out, 3); }
  }
  if (lam_out) {   // Lambda_eta = Tinv^T diag(lam) Tinv (k_cam_prep keeps the block, not lam): lam_c = (T^T Lambda_eta T)_cc with T = inverse(Tinv), a few u relative
    tmp.resize(3 * N);
    for (size_t k = 0; k < N; ++k) {
      const double* A = &Ti[9 * k]; const double* L6 = &Lm[6 * k];
      const double L[9] = {L6[0], L6[1], L6[2], L6[1], L6[3], L6[4], L6[2], L6[4], L6[5]};
      const double co[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                            A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                            A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
      const double det = A[0] * co[0] + A[1] * co[3] + A[2] * co[6];
      for (int cc = 0; cc < 3; ++cc) {
        const double t[3] = {co[cc] / det, co[3 + cc] / det, co[6 + cc] / det};   // column cc of T
        double v = 0.0;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) v += t[a] * L[3 * a + b] * t[b];
        tmp[3 * k + cc] = v;
      }
    }
    put(tmp.data(), lam_out, 3);
  }
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->path = s.dense_used && !s.comp_used ? GSFM_STEP_DENSE : s.comp_used ? GSFM_STEP_COMPONENTS : s.single_reduction ? GSFM_STEP_PCG_SINGLE_REDUCTION : GSFM_STEP_PCG_TEXTBOOK;
    info->cg_iterations = s.cg + s.cg_spent; info->cg_tolerance = tol_eff;
    // (the component step hands the LM loop a converged residual held against the 1e-14 rule of disconnected graphs, run_component_step:
    // what its PCG solve -- at the requested tolerance where one large component is left -- ended on is in the scalars)
    info->cg_rel = s.comp_used ? last_rel : s.cg_rel;
    info->loose_cg_iterations = c.loose_cg; info->loose_cg_rel = c.loose_rel;
    info->coarse_n = (int32_t)P->coarse_n; info->lin_is_lap = P->lin_is_lap ? 1 : 0; info->column_sorted = P->cs.active ? 1 : 0;
    info->graph_launches = P->graph_launches; info->dense_info = lm.dense_info();
    for (int k = 0; k < 5; ++k) info->step_sums[k] = lm.h[SC_STEP + k];
    info->gmax = lm.gmax; info->cost = lm.x_cost;
  }
  return GSFM_OK;
  });
}

gsfm_status gsfm_rot_dense_factor_check(int32_t schedule, uint32_t n_items, const uint32_t* n, const double* A, const double* b, const int32_t* active,
                                        double* x_out, double* L_out, int32_t* info_out) {
  return guarded("the dense factorisation check", dense_factor_check_impl, schedule, n_items, n, A, b, active, x_out, L_out, info_out);
}

gsfm_status gsfm_rot_time_kernels(gsfm_rot_problem* P, const double* rot, int32_t reps, double* out_ms4) {
  if (!P || !rot || !out_ms4 || reps <= 0) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "bad argument");
  if (P->cb) return (gsfm_status)fail(GSFM_ERR_UNSUPPORTED, "time_kernels needs a native loss");
  DeviceGuard g(P->device);
  const gsfm_rot_options o = default_options();
  if (int st = upload_state(P, rot)) return (gsfm_status)st;
  if (int st = launch_lin(P, P->q.p)) return (gsfm_status)st;
  launch_prep(P, o, o.initial_trust_region_radius, true);
  if (int st = sync_check(P, "time_kernels setup")) return (gsfm_status)st;
  for (int which = 0; which < 4; ++which) out_ms4[which] = 0.0;   // ([3]: reserved)
  for (int which = 0; which < 3; ++which) {   // two warm-ups, the faster of two rounds
    auto launch = [&] { return which == 0 ? launch_cost(P, P->q.p, SC_COST) : which == 1 ? launch_lin(P, P->q.p) : launch_matvec(P, P->Mblk.p, P->b.p, P->Ap.p, nullptr); };
    if (int st = timed(P, reps, 2, 2, "time_kernels", launch, &out_ms4[which])) return (gsfm_status)st;
  }
  return GSFM_OK;
}

gsfm_status gsfm_rot_matvec_bytes(gsfm_rot_problem* P, double* layout_bytes, double* lin_bytes, int32_t* form) {
  if (!P) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL problem");
  const double N = (double)P->n_rows;
  const bool lap = P->lap_capable;
  if (lap && P->cs.active) {
    // mat-vec, per position: its 2-, 4- or 6-byte record (column | slot | row count; 2: delta-coded, ColLayoutDev::k16) + body-frame block 48; partial sums written and
    // read once; the gathered vector, the diagonal blocks, p, q in, y out once per camera.  Linearisation, per position: record 8 +
    // q_rel 32 + whitening 48 in, block 48 out; nine partial sums per row and workgroup
    if (layout_bytes) *layout_bytes = (P->cs.k16_active ? 50.0 : P->cs.cmax ? 52.0 : 54.0) * (double)P->cs.n_pos + 2.0 * 24.0 * P->cs.n_wg * GSFM_COL_RB + (24.0 + 48.0 + 24.0 + 32.0 + 24.0) * N;
    if (lin_bytes) *lin_bytes = (8.0 + (P->q3 ? 24.0 : 32.0) + (P->wmode == W_MATRIX ? 48.0 : P->wmode == W_SCALAR ? 8.0 : 0.0) + 48.0) * (double)P->cs.n_pos + 2.0 * 72.0 * P->cs.n_wg * GSFM_COL_RB + (32.0 + 72.0) * N;
    if (form) *form = 2;
  } else {
    if (layout_bytes) *layout_bytes = (double)P->dir.n * (lap ? 52.0 : 76.0) + 2.0 * 24.0 * N;
    const double w = P->wmode == W_MATRIX ? 48.0 : P->wmode == W_SCALAR ? 8.0 : 0.0;
    if (lin_bytes) *lin_bytes = (double)P->dir.n * (4.0 + (P->q3 ? 24.0 : 32.0) + w + (lap ? 48.0 : 72.0)) + (32.0 + 72.0) * N;
    if (form) *form = lap ? 1 : 0;
  }
  return GSFM_OK;
}

gsfm_status gsfm_rot_sweep_bytes(gsfm_rot_problem* P, double* algorithmic, double* layout) {
  if (!P) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL problem");
  // indices 8 B + measurement 24 B (32 B for the quaternion types) + whitening 48/8/0 B + weight out 8 B
  const double w = P->wmode == W_MATRIX ? 48.0 : P->wmode == W_SCALAR ? 8.0 : 0.0;
  if (algorithmic) *algorithmic = 8.0 + (P->functor == F_AA ? 24.0 : 32.0) + w + 8.0;
  // as laid out: uint2 idx + the measurement (24 B on the W_MATRIX problems of >= 1 M edges since round 6: three quaternion components, edge_math.hpp qrel_three; 32 B otherwise) + whitening planes; the weight is consumed in-kernel (no per-edge store)
  if (layout) *layout = 8.0 + (P->q3 ? 24.0 : 32.0) + w;
  return GSFM_OK;
}

gsfm_status gsfm_cov_estimate(uint64_t n_edges, const uint64_t* match_ptr, const double* matches, const double* intrinsics,
                              const double* rot_in, const double* trans_in, int32_t max_iterations, double* cov9_out,
                              double* rot_out, double* trans_out, int32_t* status_out, int32_t* iters_out, double* kernel_ms) {
  return guarded("the covariance estimator", cov_estimate_impl, n_edges, match_ptr, matches, intrinsics, rot_in, trans_in, max_iterations, cov9_out,
                 rot_out, trans_out, status_out, iters_out, kernel_ms);
}

int32_t gsfm_magsac_table(int32_t nu, double* out, int32_t cap) {
  if (nu != 3 && nu != 4 && nu != 9) return -1;
  const std::vector<double>& t = magsac_table(nu);
  const int m = std::min((int)t.size(), cap);
  if (out && m > 0) std::memcpy(out, t.data(), 8 * (size_t)m);
  return (int)t.size();
}
gsfm_status gsfm_magsac_constants(int32_t nu, double* C, double* q, double* gk) {
  if (nu != 3 && nu != 4 && nu != 9) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "nu must be 3, 4 or 9");
  const MagsacConst c = magsac_const(nu);
  if (C) *C = c.C; if (q) *q = c.q; if (gk) *gk = c.gk;
  return GSFM_OK;
}

}  // extern "C"
