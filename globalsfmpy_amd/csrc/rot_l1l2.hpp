// Host side of the robust L1 + IRLS rotation estimator (include/gsfm_rot_l1l2.h): the refusals, the host structure
// (rot_l1l2_structure.hpp), one device slab and a private stream (flat_call.hpp), and the control of the two stages over the kernels of
// rot_l1l2_kernels.hpp.  The linear solves run through lm_loop.hpp's pcg_loop.  The host looks at the device scalars through a mapped
// mailbox (L1Mail): once per cg_check_interval PCG iterations, once per ADMM iteration (the six norms) and once per outer or IRLS
// iteration (the step size).  Nothing is kept between calls.  Part of libgsfm_rot.so's one translation unit.
#pragma once
#include "host_common.hpp"
#include "flat_call.hpp"
#include "lm_loop.hpp"
#include "rot_l1l2_structure.hpp"
#include "rot_l1l2_kernels.hpp"
#include "../../include/gsfm_rot_l1l2.h"

namespace {

static_assert(L1S_RZ0 == PCG_RZ0 && L1S_RZA == PCG_RZA && L1S_RZB == PCG_RZB, "the first device scalars are pcg_loop's");

// the device scalars in mapped host memory, the stamp behind them
struct L1Mail {
  double* host = nullptr; double* dev = nullptr;
  hipEvent_t ev = nullptr;
  unsigned long long stamp = 0;
  ~L1Mail() { if (ev) (void)hipEventDestroy(ev); if (host) (void)hipHostFree(host); }
  int open() {
    HIPCHK(hipHostMalloc((void**)&host, (L1S_N + 1) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(host, 0, (L1S_N + 1) * sizeof(double));
    HIPCHK(hipHostGetDevicePointer((void**)&dev, host, 0));
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return 0;
  }
  // enqueue the post of the scalars and wait for it; out[L1S_N]
  int look(hipStream_t s, const double* scal, double* out) {
    hipLaunchKernelGGL(k_l1_post, dim3(1), dim3(1), 0, s, scal, (int)L1S_N, dev, (unsigned long long*)(dev + L1S_N), ++stamp);
    HIPCHK(hipEventRecord(ev, s));
    HIPCHK(hipEventSynchronize(ev));
    if (__atomic_load_n((unsigned long long*)(host + L1S_N), __ATOMIC_ACQUIRE) != stamp)
      return fail(GSFM_ERR_HIP, std::string("the robust rotation estimator's device scalars never arrived: ") + hipGetErrorString(hipGetLastError()));
    for (int k = 0; k < L1S_N; ++k) out[k] = host[k];
    return 0;
  }
};

gsfm_rot_l1l2_options l1_options(const gsfm_rot_l1l2_options* opt) {
  gsfm_rot_l1l2_options o;
  if (opt) return *opt;
  gsfm_rot_l1l2_options_default(&o);
  return o;
}

// The refusals of include/gsfm_rot_l1l2.h, before any device call.  rot_aa may be NULL (the Laplacian aid); graph: fixed_cam and the
// connectivity are checked too.
int l1_check(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, const double* rot_aa,
             int32_t fixed_cam, bool graph) {
  if (n_cams == 0 || n_edges == 0) return fail(GSFM_ERR_EMPTY, "no cameras or no edges");
  if (!edge_i || !edge_j) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (n_edges >= (1ull << 31) || n_cams >= (1u << 31)) return fail(GSFM_ERR_INVALID_ARG, "problem too large (2^31 edges or cameras)");
  for (uint64_t e = 0; e < n_edges; ++e) {
    if (edge_i[e] >= n_cams || edge_j[e] >= n_cams) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has a camera index >= n_cams");
    if (edge_i[e] == edge_j[e]) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " joins camera " + std::to_string(edge_i[e]) + " to itself");
  }
  if (rel_aa)
    for (uint64_t t = 0; t < 3 * n_edges; ++t)
      if (!std::isfinite(rel_aa[t])) return fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(t / 3) + " has a non-finite relative rotation");
  std::vector<uint8_t> has_edge(n_cams, 0);
  for (uint64_t e = 0; e < n_edges; ++e) has_edge[edge_i[e]] = has_edge[edge_j[e]] = 1;
  if (rot_aa)
    for (uint32_t k = 0; k < n_cams; ++k)
      if (has_edge[k] && !(std::isfinite(rot_aa[3 * (size_t)k]) && std::isfinite(rot_aa[3 * (size_t)k + 1]) && std::isfinite(rot_aa[3 * (size_t)k + 2])))
        return fail(GSFM_ERR_INVALID_ARG, "camera " + std::to_string(k) + " has an edge and a non-finite start rotation");
  if (!graph) return 0;
  if (fixed_cam < 0 || (int64_t)fixed_cam >= (int64_t)n_cams) return fail(GSFM_ERR_INVALID_ARG, "fixed_cam must be a camera index < n_cams");
  if (!has_edge[fixed_cam]) return fail(GSFM_ERR_INVALID_ARG, "fixed_cam " + std::to_string(fixed_cam) + " appears in no edge");
  const int64_t lost = l1_first_unreachable(n_cams, n_edges, edge_i, edge_j, (uint32_t)fixed_cam);
  if (lost >= 0)
    return fail(GSFM_ERR_INVALID_ARG, "camera " + std::to_string(lost) + " has an edge but is not connected to fixed_cam " + std::to_string(fixed_cam) +
                                          ": the view graph must be one component");
  return 0;
}

constexpr int L1_PRODUCT_REPS = 20;   // products timed back to back by the Laplacian aid

// One call's device state.  rot: true for the solve and the residual aid (rotations, measurements and the edge vectors are laid out too)
struct L1Call {
  FlatCall fc;
  L1Mail mail;
  size_t N = 0, E = 0;
  uint32_t n_short = 0, n_long = 0, nb_short = 0, nb_long = 0, nb_rows = 0, nb_edge = 0, nb_vec = 0, nb_cam = 0, P = 0;
  double n_free = 0.0;
  uint32_t *ei = nullptr, *ej = nullptr, *pos_i = nullptr, *pos_j = nullptr, *row_ptr = nullptr, *nbr = nullptr, *ent = nullptr, *short_rows = nullptr, *long_rows = nullptr;
  uint8_t *active = nullptr, *touched = nullptr;
  Quat *q = nullptr, *qrel = nullptr;
  double *rot = nullptr, *rel = nullptr, *b = nullptr, *z = nullptr, *u = nullptr, *v = nullptr, *dz = nullptr, *wd = nullptr, *wedge = nullptr, *deg1 = nullptr,
         *degw = nullptr, *rhs = nullptr, *r = nullptr, *zz = nullptr, *p = nullptr, *Ap = nullptr, *y = nullptr, *part = nullptr, *scal = nullptr;
  double hs[L1S_N] = {};
  std::vector<uint8_t> h_active;

  static uint32_t blocks(size_t n, size_t per = 256) { return (uint32_t)std::max<size_t>(1, std::min<size_t>((n + per - 1) / per, GSFM_L1_MAX_BLOCKS)); }

  // lay out, commit and upload the structure; rot / rel may be NULL without `rot`
  int open(const L1Structure& S, uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, uint32_t fixed_cam, bool with_rot,
           const double* rel_aa, const double* rot_aa, const char* who, int n_spans = 1) {
    N = n_cams; E = n_edges;
    const size_t ND = 2 * E;
    n_short = (uint32_t)S.short_rows.size(); n_long = (uint32_t)S.long_rows.size();
    nb_short = (n_short + 31) / 32; nb_long = (n_long + 3) / 4; nb_rows = std::max(1u, nb_short + nb_long);
    nb_edge = blocks(E); nb_vec = blocks(3 * N); nb_cam = blocks(N);
    P = std::max(std::max(nb_rows, nb_edge), std::max(nb_vec, nb_cam));
    n_free = (double)S.n_present - 1.0;
    SlabTake take{FlatLayout(), nullptr};
    auto place = [&](SlabTake& t) {
      // the vectors that must be zero off the free cameras come first, side by side: one memset clears them
      for (double** vec : {&rhs, &r, &zz, &p, &Ap, &y}) t(*vec, 3 * N);
      t(touched, N); t(scal, (size_t)L1S_N);
      const size_t zeroed = t.L.total;
      t(ei, E); t(ej, E); t(pos_i, E); t(pos_j, E); t(row_ptr, N + 1); t(nbr, ND); t(ent, ND); t(short_rows, (size_t)n_short); t(long_rows, (size_t)n_long);
      t(active, N); t(deg1, N); t(degw, N); t(wd, ND); t(wedge, E); t(part, 4 * (size_t)P);
      if (with_rot) { t(q, N); t(qrel, E); t(rot, 3 * N); t(rel, 3 * E); for (double** vec : {&b, &z, &u, &v, &dz}) t(*vec, 3 * E); }
      return zeroed;
    };
    place(take);
    if (int st = fc.commit(take.L, who, n_spans)) return st;
    if (int st = mail.open()) return st;
    SlabTake fill{FlatLayout(), fc.slab};
    const size_t zeroed = place(fill);
    const hipStream_t s = fc.s;
    HIPCHK(hipMemsetAsync(fc.slab, 0, zeroed, s));
    h_active = S.present; h_active[fixed_cam] = 0;
    auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    HIPCHK(up(ei, edge_i, 4 * E)); HIPCHK(up(ej, edge_j, 4 * E)); HIPCHK(up(pos_i, S.pos_i.data(), 4 * E)); HIPCHK(up(pos_j, S.pos_j.data(), 4 * E));
    HIPCHK(up(row_ptr, S.row_ptr.data(), 4 * (N + 1))); HIPCHK(up(nbr, S.nbr.data(), 4 * ND)); HIPCHK(up(ent, S.ent.data(), 4 * ND));
    HIPCHK(up(short_rows, S.short_rows.data(), 4 * (size_t)n_short)); HIPCHK(up(long_rows, S.long_rows.data(), 4 * (size_t)n_long));
    HIPCHK(up(active, h_active.data(), N)); HIPCHK(up(deg1, S.degree.data(), 8 * N)); HIPCHK(up(degw, S.degree.data(), 8 * N));
    if (with_rot) { HIPCHK(up(rot, rot_aa, 24 * N)); HIPCHK(up(rel, rel_aa, 24 * E)); }
    return 0;
  }

  void reduce(uint32_t n, int m, int slot) { hipLaunchKernelGGL(k_l1_reduce, dim3(1), dim3(256), 0, fc.s, (const double*)part, n, P, m, scal + slot); }
  int look() { return mail.look(fc.s, scal, hs); }

  void setup() {
    hipLaunchKernelGGL(k_l1_setup, dim3((unsigned)((std::max(N, E) + 255) / 256)), dim3(256), 0, fc.s, (uint32_t)N, (uint32_t)E, (const double*)rot, (const double*)rel, q, qrel);
  }
  // b at the current rotations; weights: also w b (in v), and w at the directed entries
  void residuals(double sigma, bool weights, double* sq = nullptr, double* w = nullptr) {
    hipLaunchKernelGGL(k_l1_resid, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, fc.s, (uint32_t)E, (const uint32_t*)ei, (const uint32_t*)ej, (const Quat*)q,
                       (const Quat*)qrel, sigma, (const uint32_t*)pos_i, (const uint32_t*)pos_j, b, sq, w, weights ? v : nullptr, weights ? wd : nullptr);
  }
  // rhs = A^T v0 on the free cameras; NV = 3: also the two camera norms into scal[L1S_S2], scal[L1S_ATU2]; NV = 1 with weights: degw
  template <int NV> void rows(const double* v0, const double* v1, const double* v2, bool weights, double rho) {
    const double* w = weights ? wd : nullptr;
    if (n_short) hipLaunchKernelGGL((k_l1_rows<NV, 8>), dim3(nb_short), dim3(256), 0, fc.s, (const uint32_t*)short_rows, n_short, (const uint32_t*)row_ptr,
                                    (const uint32_t*)ent, v0, v1, v2, w, rhs, degw, rho, part, 0u, P);
    if (n_long) hipLaunchKernelGGL((k_l1_rows<NV, 64>), dim3(nb_long), dim3(256), 0, fc.s, (const uint32_t*)long_rows, n_long, (const uint32_t*)row_ptr,
                                   (const uint32_t*)ent, v0, v1, v2, w, rhs, degw, rho, part, nb_short, P);
    if (NV == 3) reduce(nb_short + nb_long, 2, L1S_S2);
  }
  template <bool W> void matvec() {
    const double* d = W ? degw : deg1;
    if (n_short) hipLaunchKernelGGL((k_l1_matvec<W, 8>), dim3(nb_short), dim3(256), 0, fc.s, (const uint32_t*)short_rows, n_short, (const uint32_t*)row_ptr,
                                    (const uint32_t*)nbr, (const double*)wd, d, (const double*)p, Ap, part, 0u);
    if (n_long) hipLaunchKernelGGL((k_l1_matvec<W, 64>), dim3(nb_long), dim3(256), 0, fc.s, (const uint32_t*)long_rows, n_long, (const uint32_t*)row_ptr,
                                   (const uint32_t*)nbr, (const double*)wd, d, (const double*)p, Ap, part, nb_short);
    reduce(nb_short + nb_long, 1, L1S_PAP);
  }
  // y = L^-1 rhs from y = 0 (L weighted: by wd and degw): lm_loop.hpp's driver with the breakdown rule
  int pcg(bool weighted, const gsfm_rot_l1l2_options& o, int* iters, bool* stalled, double* rel_out) {
    const size_t n3 = 3 * N;
    const double* d = weighted ? degw : deg1;
    const hipStream_t s = fc.s;
    hipLaunchKernelGGL(k_l1_pcg_start, dim3(nb_vec), dim3(256), 0, s, n3, (const double*)rhs, d, r, zz, p, y, part);
    reduce(nb_vec, 1, L1S_RZ0);
    HIPCHK(hipMemcpyAsync(scal + L1S_RZA, scal + L1S_RZ0, 8, hipMemcpyDeviceToDevice, s));
    auto iterate = [&](int cur, int nxt) {
      if (weighted) matvec<true>(); else matvec<false>();
      hipLaunchKernelGGL(k_l1_pcg_update, dim3(nb_vec), dim3(256), 0, s, n3, (const double*)scal, cur, (const double*)p, (const double*)Ap, d, y, r, zz, part);
      reduce(nb_vec, 1, nxt);
      hipLaunchKernelGGL(k_l1_pcg_dir, dim3(nb_vec), dim3(256), 0, s, n3, (const double*)scal, nxt, cur, (const double*)zz, p);
    };
    auto read = [&](int slot, double* val) { if (int st = look()) return st; *val = hs[slot]; return 0; };
    return pcg_loop(o, true, iterate, read, iters, stalled, rel_out);
  }
  // ... counted into the summary
  int solve_linear(bool weighted, const gsfm_rot_l1l2_options& o, gsfm_rot_l1l2_summary* sum) {
    int iters = 0; bool stalled = false; double rel_res = 0.0;
    if (int st = pcg(weighted, o, &iters, &stalled, &rel_res)) return st;
    sum->num_linear_solves++; sum->num_cg_iterations += iters;
    if (stalled) sum->num_pcg_stalled_solves++;
    if (!(rel_res <= sum->worst_accepted_cg_residual)) sum->worst_accepted_cg_residual = rel_res;   // (a NaN is kept)
    return 0;
  }
  // R_k <- R_k Exp(y_k), b there (weights: and the IRLS weights), and the look: *avg = mean |y_k| over the free cameras
  int step(double sigma, bool weights, double* avg) {
    hipLaunchKernelGGL(k_l1_update, dim3(nb_cam), dim3(256), 0, fc.s, (uint32_t)N, (const uint8_t*)active, (const double*)y, q, touched, part);
    reduce(nb_cam, 1, L1S_STEP);
    residuals(sigma, weights);
    if (int st = look()) return st;
    *avg = hs[L1S_STEP] / n_free;
    return 0;
  }
};

int l1_stage_l1(L1Call& c, const gsfm_rot_l1l2_options& o, gsfm_rot_l1l2_summary* sum) {
  const hipStream_t s = c.fc.s;
  const size_t E = c.E;
  const double eps_pri_abs = std::sqrt(3.0 * (double)E) * o.admm_absolute_tolerance, eps_dual_abs = std::sqrt(3.0 * c.n_free) * o.admm_absolute_tolerance;
  int inner = o.admm_initial_iterations;
  for (int outer = 0; outer < o.max_num_l1_iterations; ++outer) {
    HIPCHK(hipMemsetAsync(c.z, 0, 24 * E, s));
    HIPCHK(hipMemsetAsync(c.u, 0, 24 * E, s));
    c.rows<1>(c.b, nullptr, nullptr, false, o.admm_rho);   // A^T (b + z - u) at z = u = 0
    int it = 0;
    while (it < inner) {
      if (int st = c.solve_linear(false, o, sum)) return st;
      hipLaunchKernelGGL(k_l1_admm_edge, dim3(c.nb_edge), dim3(256), 0, s, (uint32_t)E, (const uint32_t*)c.ei, (const uint32_t*)c.ej, (const double*)c.y,
                         (const double*)c.b, c.z, c.u, c.v, c.dz, o.admm_rho, o.admm_alpha, c.part, c.P);
      c.reduce(c.nb_edge, 4, L1S_R2);
      c.rows<3>(c.v, c.dz, c.u, false, o.admm_rho);
      if (int st = c.look()) return st;
      ++it;
      const double r_norm = std::sqrt(c.hs[L1S_R2]), s_norm = std::sqrt(c.hs[L1S_S2]);
      const double eps_pri = eps_pri_abs + o.admm_relative_tolerance * std::sqrt(std::fmax(c.hs[L1S_AX2], std::fmax(c.hs[L1S_Z2], c.hs[L1S_B2])));
      const double eps_dual = eps_dual_abs + o.admm_relative_tolerance * std::sqrt(c.hs[L1S_ATU2]);
      if (o.verbose) fprintf(stderr, "[gsfm l1l2] outer %d admm %3d |r| %.6e eps %.6e |s| %.6e eps %.6e\n", outer, it, r_norm, eps_pri, s_norm, eps_dual);
      if (!std::isfinite(r_norm) || !std::isfinite(s_norm) || !std::isfinite(eps_pri) || !std::isfinite(eps_dual)) { sum->nonfinite = 1; break; }
      if (r_norm < eps_pri && s_norm < eps_dual) break;
    }
    double avg = 0.0;
    if (int st = c.step(o.irls_loss_parameter_sigma, false, &avg)) return st;
    sum->num_l1_iterations = outer + 1;
    if (outer < GSFM_ROT_L1L2_MAX_L1) { sum->num_admm_iterations[outer] = it; sum->l1_step[outer] = avg; }
    if (o.verbose) fprintf(stderr, "[gsfm l1l2] outer %d: %d admm iterations, avg step %.9e\n", outer, it, avg);
    if (!std::isfinite(avg)) sum->nonfinite = 1;
    if (sum->nonfinite) return 0;
    if (avg <= o.l1_step_convergence_threshold) { sum->l1_converged = 1; break; }
    inner *= 2;
  }
  return 0;
}

int l1_stage_irls(L1Call& c, const gsfm_rot_l1l2_options& o, gsfm_rot_l1l2_summary* sum) {
  c.residuals(o.irls_loss_parameter_sigma, true);
  for (int it = 0; it < o.max_num_irls_iterations; ++it) {
    c.rows<1>(c.v, nullptr, nullptr, true, 1.0);   // A^T W b and the weighted degree
    if (int st = c.solve_linear(true, o, sum)) return st;
    double avg = 0.0;
    if (int st = c.step(o.irls_loss_parameter_sigma, true, &avg)) return st;
    sum->num_irls_iterations = it + 1; sum->last_irls_step = avg;
    if (o.verbose) fprintf(stderr, "[gsfm l1l2] irls %3d avg step %.9e\n", it, avg);
    if (!std::isfinite(avg)) { sum->nonfinite = 1; return 0; }
    if (avg < o.irls_step_convergence_threshold) { sum->irls_converged = 1; break; }
  }
  return 0;
}

gsfm_status l1l2_solve_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, double* rot_aa,
                            int32_t fixed_cam, const gsfm_rot_l1l2_options* opt, gsfm_rot_l1l2_summary* summary) {
  gsfm_rot_l1l2_summary local;
  if (!summary) summary = &local;
  std::memset(summary, 0, sizeof(*summary));
  if (n_edges && (!rel_aa || !rot_aa)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = l1_check(n_cams, n_edges, edge_i, edge_j, rel_aa, rot_aa, fixed_cam, true)) return (gsfm_status)st;
  const gsfm_rot_l1l2_options o = l1_options(opt);
  if (!(o.admm_rho > 0.0) || !(o.irls_loss_parameter_sigma > 0.0) || o.admm_initial_iterations < 1)
    return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "admm_rho and irls_loss_parameter_sigma must be positive, admm_initial_iterations at least 1");
  if (const char* why = no_device_reason("gsfm_rot_l1l2_solve")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  const double t0 = now_ms();
  summary->num_edges_used = n_edges;
  const L1Structure S = l1_build_structure(n_cams, n_edges, edge_i, edge_j, (uint32_t)fixed_cam);
  L1Call c;
  if (int st = c.open(S, n_cams, n_edges, edge_i, edge_j, (uint32_t)fixed_cam, true, rel_aa, rot_aa, "the robust rotation estimator")) return (gsfm_status)st;
  HIPCHK_S(c.fc.begin_span());
  c.setup();
  c.residuals(o.irls_loss_parameter_sigma, false);
  if (int st = l1_stage_l1(c, o, summary)) return (gsfm_status)st;
  if (!summary->nonfinite)
    if (int st = l1_stage_irls(c, o, summary)) return (gsfm_status)st;
  hipLaunchKernelGGL(k_l1_finish, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, c.fc.s, n_cams, (const Quat*)c.q, (const uint8_t*)c.touched, c.rot);
  HIPCHK_S(c.fc.end_span());
  std::vector<double> out(3 * (size_t)n_cams);
  HIPCHK_S(hipMemcpyAsync(out.data(), c.rot, 24 * (size_t)n_cams, hipMemcpyDeviceToHost, c.fc.s));
  HIPCHK_S(c.fc.sync());
  std::memcpy(rot_aa, out.data(), 24 * (size_t)n_cams);
  summary->kernel_ms = c.fc.kernel_ms();
  summary->t_total_ms = now_ms() - t0;
  return GSFM_OK;
}

gsfm_status l1l2_residuals_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, const double* rot_aa,
                                const gsfm_rot_l1l2_options* opt, double* b_out, double* sq_out, double* weight_out) {
  if (n_edges && (!rel_aa || !rot_aa || !b_out)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = l1_check(n_cams, n_edges, edge_i, edge_j, rel_aa, rot_aa, 0, false)) return (gsfm_status)st;
  const gsfm_rot_l1l2_options o = l1_options(opt);
  if (const char* why = no_device_reason("gsfm_rot_l1l2_residuals")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  const L1Structure S = l1_build_structure(n_cams, n_edges, edge_i, edge_j, edge_i[0]);
  L1Call c;
  if (int st = c.open(S, n_cams, n_edges, edge_i, edge_j, edge_i[0], true, rel_aa, rot_aa, "the residuals of the robust rotation estimator")) return (gsfm_status)st;
  c.setup();
  // |b|^2 and the weight per edge land in the edge vectors z and u, which this call does not use otherwise
  c.residuals(o.irls_loss_parameter_sigma, true, c.z, c.u);
  HIPCHK_S(hipMemcpyAsync(b_out, c.b, 24 * (size_t)n_edges, hipMemcpyDeviceToHost, c.fc.s));
  if (sq_out) HIPCHK_S(hipMemcpyAsync(sq_out, c.z, 8 * (size_t)n_edges, hipMemcpyDeviceToHost, c.fc.s));
  if (weight_out) HIPCHK_S(hipMemcpyAsync(weight_out, c.u, 8 * (size_t)n_edges, hipMemcpyDeviceToHost, c.fc.s));
  HIPCHK_S(c.fc.sync());
  return GSFM_OK;
}

gsfm_status l1l2_laplacian_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* weights, int32_t fixed_cam,
                                const double* rhs, const gsfm_rot_l1l2_options* opt, double* x_out, double* info_out) {
  if (!rhs || !x_out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  if (int st = l1_check(n_cams, n_edges, edge_i, edge_j, nullptr, nullptr, fixed_cam, true)) return (gsfm_status)st;
  if (weights)
    for (uint64_t e = 0; e < n_edges; ++e)
      if (!(weights[e] > 0.0) || !std::isfinite(weights[e])) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "edge " + std::to_string(e) + " has a weight that is not positive and finite");
  const gsfm_rot_l1l2_options o = l1_options(opt);
  if (const char* why = no_device_reason("gsfm_rot_l1l2_laplacian_solve")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);
  const L1Structure S = l1_build_structure(n_cams, n_edges, edge_i, edge_j, (uint32_t)fixed_cam);
  L1Call c;
  if (int st = c.open(S, n_cams, n_edges, edge_i, edge_j, (uint32_t)fixed_cam, false, nullptr, nullptr, "the Laplacian solve of the robust rotation estimator", 2)) return (gsfm_status)st;
  const size_t N = n_cams;
  std::vector<double> h_rhs(3 * N, 0.0), h_deg;
  for (size_t k = 0; k < N; ++k)
    if (c.h_active[k]) for (int d = 0; d < 3; ++d) h_rhs[3 * k + d] = rhs[3 * k + d];
  HIPCHK_S(hipMemcpyAsync(c.rhs, h_rhs.data(), 24 * N, hipMemcpyHostToDevice, c.fc.s));
  if (weights) {
    // the weighted degree in the row's order, as the row kernel sums it on the way to a solve's IRLS system
    HIPCHK_S(hipMemcpyAsync(c.wedge, weights, 8 * (size_t)n_edges, hipMemcpyHostToDevice, c.fc.s));
    hipLaunchKernelGGL(k_l1_spread, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, c.fc.s, (uint32_t)n_edges, (const double*)c.wedge, (const uint32_t*)c.pos_i,
                       (const uint32_t*)c.pos_j, c.wd);
    h_deg = S.degree;
    for (size_t k = 0; k < N; ++k) {
      if (!c.h_active[k]) continue;
      double d = 0.0;
      for (uint32_t t = S.row_ptr[k]; t < S.row_ptr[k + 1]; ++t) d += weights[S.ent[t] >> 1];
      h_deg[k] = d;
    }
    HIPCHK_S(hipMemcpyAsync(c.degw, h_deg.data(), 8 * N, hipMemcpyHostToDevice, c.fc.s));
  }
  int iters = 0; bool stalled = false; double rel_res = 0.0;
  HIPCHK_S(c.fc.begin_span());
  if (int st = c.pcg(weights != nullptr, o, &iters, &stalled, &rel_res)) return (gsfm_status)st;
  HIPCHK_S(c.fc.end_span());
  HIPCHK_S(hipMemcpyAsync(x_out, c.y, 24 * N, hipMemcpyDeviceToHost, c.fc.s));
  // the product alone, for the timing tool: L1_PRODUCT_REPS launches back to back on the last search direction
  if (info_out) {
    HIPCHK_S(c.fc.begin_span());
    for (int k = 0; k < L1_PRODUCT_REPS; ++k) { if (weights) c.matvec<true>(); else c.matvec<false>(); }
    HIPCHK_S(c.fc.end_span());
  }
  HIPCHK_S(c.fc.sync());
  if (info_out) {
    float solve_ms = 0.0f, product_ms = 0.0f;
    (void)hipEventElapsedTime(&solve_ms, c.fc.ev[0], c.fc.ev[1]);
    (void)hipEventElapsedTime(&product_ms, c.fc.ev[2], c.fc.ev[3]);
    const double n_rows = (double)c.n_short + (double)c.n_long;
    info_out[0] = iters; info_out[1] = stalled ? 1.0 : 0.0; info_out[2] = rel_res; info_out[3] = solve_ms;
    info_out[4] = product_ms / L1_PRODUCT_REPS;
    // what one product streams: per directed entry the neighbour (and the weight), per free row its list entry, two row pointers'
    // worth of offsets, the degree, p_k and y_k; the gathered p_m (24 B per entry) comes from the caches and is not counted
    info_out[5] = 2.0 * (double)n_edges * (weights ? 12.0 : 4.0) + n_rows * (4.0 + 8.0 + 8.0 + 24.0 + 24.0);
  }
  return GSFM_OK;
}

}  // namespace

extern "C" {

int gsfm_rot_l1l2_abi_version(void) { return GSFM_ROT_L1L2_ABI_VERSION; }

void gsfm_rot_l1l2_options_default(gsfm_rot_l1l2_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->max_num_l1_iterations = 5; o->max_num_irls_iterations = 100;
  o->l1_step_convergence_threshold = 1e-3; o->irls_step_convergence_threshold = 1e-3;
  o->irls_loss_parameter_sigma = 5.0 * 3.14159265358979323846 / 180.0;
  o->admm_initial_iterations = 5; o->max_cg_iterations = 2000;
  o->admm_rho = 1.0; o->admm_alpha = 1.0; o->admm_absolute_tolerance = 1e-4; o->admm_relative_tolerance = 1e-2;
  o->cg_relative_tolerance = 1e-14; o->cg_check_interval = 4; o->cg_stall_iterations = 200; o->verbose = 0;
}

gsfm_status gsfm_rot_l1l2_solve(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, double* rot_aa_inout,
                                int32_t fixed_cam, const gsfm_rot_l1l2_options* options, gsfm_rot_l1l2_summary* summary) {
  return guarded("the robust rotation estimator", l1l2_solve_impl, n_cams, n_edges, edge_i, edge_j, rel_aa, rot_aa_inout, fixed_cam, options, summary);
}
gsfm_status gsfm_rot_l1l2_residuals(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa, const double* rot_aa,
                                    const gsfm_rot_l1l2_options* options, double* b_out, double* sq_out, double* weight_out) {
  return guarded("the residuals of the robust rotation estimator", l1l2_residuals_impl, n_cams, n_edges, edge_i, edge_j, rel_aa, rot_aa, options, b_out, sq_out, weight_out);
}
gsfm_status gsfm_rot_l1l2_laplacian_solve(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* weights, int32_t fixed_cam,
                                          const double* rhs, const gsfm_rot_l1l2_options* options, double* x_out, double* info_out) {
  return guarded("the Laplacian solve of the robust rotation estimator", l1l2_laplacian_impl, n_cams, n_edges, edge_i, edge_j, weights, fixed_cam, rhs, options, x_out, info_out);
}

}  // extern "C"
