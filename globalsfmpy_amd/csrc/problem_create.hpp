// Host side, part 6: gsfm_rot_problem_create -- replaces the edge loop that fills the ceres::Problem (estimator.cpp:47-65, 110-166, 228-295).
// problem_create_impl is a sequence of phases: the host structure (host_structure.hpp: rows, relabelling, cost tiles, column-sorted layout),
// the choices taken from it, uploads, whitening, camera buffers, the sharded create-time agreement (CreateCtx).
#pragma once
#include "host_structure.hpp"

namespace {

gsfm_rot_options default_options() { gsfm_rot_options o; gsfm_rot_options_default(&o); return o; }

// What an error type asks of the problem: the functor of its residual, how its residual is weighted, which per-edge inputs it needs.
struct ErrorTypeInfo { int functor, wmode; bool need_cov, need_inl; };
ErrorTypeInfo classify_error_type(int32_t error_type) {
  switch (error_type) {
    case GSFM_ROT_QUATERNION_NORM:        return {F_QNORM, W_NONE, false, false};
    case GSFM_ROT_ROTATION_MAT_FNORM:     return {F_RFNORM, W_NONE, false, false};
    case GSFM_ROT_QUATERNION_COSINE:      return {F_QCOS, W_NONE, false, false};
    case GSFM_ROT_ANGLE_AXIS_COVARIANCE:  return {F_AA, W_MATRIX, true, false};
    case GSFM_ROT_ANGLE_AXIS_INLIERS:     return {F_AA, W_SCALAR, false, true};
    case GSFM_ROT_ANGLE_AXIS_COV_INLIERS: return {F_AA, W_MATRIX, true, true};
    case GSFM_ROT_ANGLE_AXIS_COVTRACE:
    case GSFM_ROT_ANGLE_AXIS_COVNORM:     return {F_AA, W_SCALAR, true, false};
    default:                              return {F_AA, W_NONE, false, false};   // GSFM_ROT_ANGLE_AXIS
  }
}

template <typename EidVec>
int upload_planes(gsfm_rot_problem* P, EdgePlanes& pl, const EidVec& eid, const double* d_rel_aa) {
  pl.n = eid.size();
  // (qr1: the third stored component, one double per position, on the W_MATRIX problems -- edge_math.hpp, qrel_three; the full quaternion's (z, w) pairs otherwise)
  const bool three = P->q3;
  if (pl.eid.upload(eid, P->stream) != hipSuccess || pl.qr0.alloc(pl.n) != hipSuccess || pl.qr1.alloc(three ? (pl.n + 1) / 2 : pl.n) != hipSuccess)
    return fail(GSFM_ERR_HIP, "uploading edge planes failed (out of memory?)");
  if (pl.n) hipLaunchKernelGGL(k_build_qrel, dim3(grid_for(pl.n)), dim3(GSFM_BLOCK), 0, P->stream, d_rel_aa, pl.eid.p, pl.n, pl.qr0.p, pl.qr1.p, three ? 1 : 0);
  if (P->wmode == W_MATRIX) {
    if (pl.w0.alloc(pl.n) != hipSuccess || pl.w1.alloc(pl.n) != hipSuccess || pl.w2.alloc(pl.n) != hipSuccess) return fail(GSFM_ERR_HIP, "alloc whitening planes");
  } else if (P->wmode == W_SCALAR) {
    if (pl.ws.alloc(pl.n) != hipSuccess) return fail(GSFM_ERR_HIP, "alloc weight plane");
  }
  return 0;
}

void run_whiten(gsfm_rot_problem* P, EdgePlanes& pl, const double* d_cov6, const double* d_inl) {
  if (P->wmode == W_NONE || pl.n == 0) return;
  WhitenArgs a{};
  a.cov6 = d_cov6; a.inl = d_inl; a.eid = pl.eid.p; a.n = pl.n; a.error_type = P->error_type;
  a.w0 = pl.w0.p; a.w1 = pl.w1.p; a.w2 = pl.w2.p; a.ws = pl.ws.p;
  hipLaunchKernelGGL(k_whiten, dim3(grid_for(pl.n)), dim3(GSFM_BLOCK), 0, P->stream, a);
}

// ---- create context: the sharded create-time agreement, the failure path, the phase timer.  Every phase that can fail returns a status and
// problem_create_impl leaves through bail(). ----
// Sharded: a rank-local failure (bad argument, bad edge, allocation, upload, loss set-up) must not leave the other ranks blocked in a
// collective.  Every rank passes through exactly ONE agreement all-reduce -- on the failure path from bail(), on the success path after
// ALL of its local work -- carrying (failed?, votes against the two-level preconditioner); all ranks give up together if any of them
// failed.  What follows the agreement are collectives only (active mask, component labels): they fail on every rank or on none.
struct CreateCtx {
  gsfm_rot_problem* P;
  gsfm_rot_problem** live;   // (for the exception path of the public wrapper)
  bool agreed = false;
  DevBuf<double> agree_buf;
  double coarse_votes_against = 0.0;
  const bool lap_on = getenv("GSFM_CREATE_TIMING") != nullptr;   // phase times of problem_create_impl on stderr
  double lap_t = now_ms();
  CreateCtx(gsfm_rot_problem* P_, gsfm_rot_problem** live_) : P(P_), live(live_) {}

  // The agreement also carries the number of edges this rank counts in the cost: their sum -- the problem's edge count, the same exact
  // double on every rank -- is what every LM decision that depends on "how many edges" is taken from (solver_lm.hpp: the staircase band of
  // the forcing schedule).  A rank-local count there would let one rank restart while the others enter a collective (round-5 advisor).
  int agree(double my_flag, double my_vote) {   // number of ranks that failed, or -1 if the agreement itself could not be run
    agreed = true;
    if (!P->sharded) return 0;
    double h[3] = {my_flag, my_vote, (double)P->cost.n};
    if (agree_buf.alloc(3) != hipSuccess || hipMemcpyAsync(agree_buf.p, h, 24, hipMemcpyHostToDevice, P->stream) != hipSuccess) return -1;
    const bool reduced = all_reduce(P, agree_buf.p, 3) == 0;
    if (read_back(P, h, agree_buf.p, 24, "the create-time agreement") != 0 || !reduced) return -1;   // (waited for either way: h is in flight)
    coarse_votes_against = h[1];
    P->cost_n_global = h[2];
    return (int)(h[0] + 0.5);
  }
  gsfm_status bail(int st) {
    if (P->sharded && !agreed) { const std::string keep = g_err; (void)agree(1.0, 1.0); g_err = keep; }
    *live = nullptr;
    gsfm_rot_problem_destroy(P);
    return (gsfm_status)st;
  }
  void lap(const char* what) { if (lap_on) { const double t = now_ms(); fprintf(stderr, "gsfm create: %-28s %8.1f ms\n", what, t - lap_t); lap_t = t; } }
};

// ---- the shard set-up: device, stream, timer, the shard descriptor.  Once P->sharded is set a failure reaches the other ranks through bail(). ----
int open_problem(gsfm_rot_problem* P, const gsfm_rot_shard* shard, bool multi_rank) {
  (void)hipGetDevice(&P->device);
  if (hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking) != hipSuccess) { P->stream = nullptr; (void)hipGetLastError(); }   // (checked below, after the shard set-up)
  else P->own_stream = true;
  P->timer.stream = P->stream; P->timer.init();
  // GSFM_FORCE_SHARD=1 keeps the collective code path alive for a single rank (tests on a 1-GPU box)
  if (multi_rank) { P->sharded = true; P->shard = *shard; }
  if (!P->own_stream) return fail(GSFM_ERR_HIP, "hipStreamCreate failed");
  return 0;
}

// ---- argument checks; arguments -> problem fields (functor, weighting, dimensions, the ownership range) ----
int set_problem_fields(gsfm_rot_problem* P, uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const double* rel_aa,
                       int32_t error_type, const double* cov6, const double* inlier_weight, const gsfm_rot_shard* shard, bool multi_rank) {
  if (multi_rank && (shard->slice_width == 0 || shard->rank < 0 || shard->rank >= shard->world_size || (uint64_t)shard->slice_width * shard->world_size < n_cams))
    return fail(GSFM_ERR_INVALID_ARG, "bad shard descriptor");
  if (n_cams == 0 || (n_edges == 0 && !multi_rank)) return fail(GSFM_ERR_EMPTY, "no cameras or no edges");
  if (n_edges > 0 && (!edge_i || !edge_j || !rel_aa)) return fail(GSFM_ERR_INVALID_ARG, "NULL edge arrays");
  if (error_type < 0 || error_type > 8) return fail(GSFM_ERR_INVALID_ARG, "unknown rotation error type");
  if (n_cams >= 0x7fffffffu || n_edges >= 0x7fffffffull) return fail(GSFM_ERR_INVALID_ARG, "problem too large for 31-bit indices");
  const ErrorTypeInfo et = classify_error_type(error_type);
  if (et.need_cov && !cov6) return fail(GSFM_ERR_INVALID_ARG, "this error type needs per-edge covariances (cov6)");
  if (et.need_inl && !inlier_weight) return fail(GSFM_ERR_INVALID_ARG, "this error type needs per-edge inlier weights");
  P->n_cams = n_cams; P->n_edges_in = n_edges; P->error_type = error_type;
  P->functor = et.functor;
  P->res_dim = gsfm_rot_residual_dim(error_type);
  P->param_dim = P->functor == F_AA ? 3 : 4;
  P->wmode = et.wmode;
  {  // the Laplacian form of the normal matrix (lin_kernels.hpp, lin_rows)
    const char* env = getenv("GSFM_LAPLACIAN");   // =0: keep the general 9-value blocks (A/B measurements)
    P->lap_capable = (P->functor == F_AA || P->functor == F_QCOS) && !(env && atoi(env) == 0);
    P->lap = P->lap_capable;
  }
  if (multi_rank) {
    P->own_begin = std::min<uint64_t>((uint64_t)shard->rank * shard->slice_width, n_cams);
    P->own_end = std::min<uint64_t>((uint64_t)(shard->rank + 1) * shard->slice_width, n_cams);
    P->n_pad = shard->slice_width * shard->world_size;
  } else { P->own_begin = 0; P->own_end = n_cams; P->n_pad = n_cams; P->shard.slice_width = n_cams; P->shard.world_size = 1; }
  P->n_rows = P->own_end - P->own_begin;
  if (hipHostMalloc(&P->pin, 512, hipHostMallocDefault) != hipSuccess) { P->pin = nullptr; (void)hipGetLastError(); }   // (read_back then copies to pageable memory)
  return 0;
}

HostStructure host_structure_input(const gsfm_rot_problem* P, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j) {
  HostStructure H;
  H.n_cams = P->n_cams; H.own_begin = P->own_begin; H.own_end = P->own_end; H.n_rows = P->n_rows; H.sharded = P->sharded;
  H.n_edges = n_edges; H.edge_i = edge_i; H.edge_j = edge_j;
  return H;
}

// Two-level preconditioner: aggregates = contiguous chunks of the camera order, which only mean something if that order is the locality
// order (adopted by relabel_rows, or coherent as given) -- GSFM_PCG_COARSE=n forces n aggregates, =0 switches it off.  Sets coarse_want /
// coarse_chunk / coarse_adaptive and allocates the coarse buffers.
void choose_coarse_space(gsfm_rot_problem* P, const HostStructure& H) {
  const uint32_t n_cams = H.n_cams;
  const char* env = getenv("GSFM_PCG_COARSE");
  int want = env && *env ? atoi(env) : -1;
  if (want < 0 && n_cams >= 4096) {   // (sharded: n_cams is the padded index space of the partition's locality order, the edges this rank's share)
    // spatially coherent in the numbering the rows now have (relabelled, or coherent as given)?  Mean index distance over a
    // sample of the edges: n/3 for a uniformly random graph, the neighbourhood radius for a coherent one
    double sum = 0.0; uint64_t cnt = 0;
    for (uint64_t e = 0; e < H.n_edges; e += 61) { sum += std::fabs((double)H.edge_i[e] - (double)H.edge_j[e]); ++cnt; }
    if (cnt == 0) { cnt = 1; sum = 0.0; }   // a rank without edges has no objection
    // What block-Jacobi cannot cope with is the DIAMETER of the graph, ~ cameras / neighbourhood radius.  Measured on coherent graphs: from a
    // ratio of ~100 the coarse space cuts the iterations 5-15x (12k cameras / radius 100: 120; 100k / 250: 400); between 32 and 100 it
    // depends on the degree (6000 cameras / 100, degree 40: 1.4x faster; 5000 / 100, degree 240: no fewer iterations, slower), so there it
    // is switched on only after a PCG solve has struggled; below, never.
    const double ratio = (double)n_cams / std::max(1.0, sum / (double)cnt);
    // one aggregate per ~256 cameras, 16 to 64 of them: more aggregates need fewer iterations but a larger dense inverse per LM step
    // (measured: 6000 cameras 16 > 64 aggregates, 100k cameras 64 > 16 and > 128)
    // (from 400k cameras a PCG iteration costs more than the 5 ms the host needs for the 384-unknown inverse: 128 aggregates there)
    want = ratio >= 32.0 ? (int)std::min<uint32_t>(n_cams >= 400000 ? 128 : 64, std::max<uint32_t>(16, n_cams / 256)) : 0;
    P->coarse_adaptive = ratio < 100.0;
  }
  if (want < 0) want = 0;
  want = std::min(want, 128);
  if (want < 2 || n_cams < 4u * (uint32_t)want) want = 0;
  if (!want) return;
  P->coarse_chunk = (n_cams + want - 1) / want;
  P->coarse_want = (n_cams + P->coarse_chunk - 1) / P->coarse_chunk;   // no empty aggregate
  const size_t nc = 3 * (size_t)P->coarse_want;
  const hipStream_t s = P->stream;
  if (P->coarseA.alloc(nc * nc) != hipSuccess || P->coarseAinv.alloc(nc * nc) != hipSuccess || P->coarse_rc.alloc_zeroed(nc, s) != hipSuccess ||
      P->coarse_xc.alloc_zeroed(nc + 1, s) != hipSuccess || P->coarse_scale.alloc_zeroed(2, s) != hipSuccess || P->coarse_part.alloc_zeroed(6 * (size_t)grid_for(n_cams), s) != hipSuccess) {
    P->coarseA.release(); P->coarse_want = 0; (void)hipGetLastError();   // (a sharded rank then votes against in the agreement: all ranks stay on block-Jacobi)
  }
}

// connected components of the view graph: counted here on one GPU; a rank of a sharded problem sees only its own edges, so the
// partitioner passes the verdict in the shard descriptor (GSFM_SHARD_DISCONNECTED) until sharded_agreement works it out
void components_on_one_gpu(gsfm_rot_problem* P, const HostStructure& H) {
  if (P->sharded) { P->n_components = (P->shard.flags & GSFM_SHARD_DISCONNECTED) ? 2 : 1; return; }
  P->n_components = std::max<uint32_t>(1, count_components(H.n_cams, H.n_edges, H.edge_i, H.edge_j));
  if (P->n_components > 1) component_labels(H.n_cams, H.n_edges, H.edge_i, H.edge_j, &P->comps.comp_of, &P->comps.size);   // (internal numbering: solver_components.hpp)
}

// lanes per camera row of the row-major kernels, from the mean degree
uint32_t row_lanes(uint32_t n_rows, size_t nd) {
  const double mean_deg = n_rows ? (double)nd / n_rows : 0.0;
  if (const char* g = getenv("GSFM_ROW_LANES")) {  // tuning override: lanes per camera row (power of two <= 64)
    const int v = atoi(g);
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) return (uint32_t)v;
  }
  return mean_deg >= 96 ? 64 : mean_deg >= 48 ? 32 : mean_deg >= 24 ? 16 : mean_deg >= 12 ? 8 : 4;
}

// the measurement planes as three quaternion components (edge_math.hpp, qrel_three): covariance-whitened problems whose sweeps are bound by the
// stream -- at least a million edges held by this process; GSFM_QREL3=0/1 overrides (tests force it on small graphs)
bool three_component_planes(int wmode, uint64_t n_edges) {
  const char* e = getenv("GSFM_QREL3");
  return GSFM_QREL3 != 0 && wmode == W_MATRIX && (e && *e ? atoi(e) != 0 : n_edges >= (uint64_t)1000000);
}

// Device half of the column-sorted layout: the layout arrays go up, col / deid are REPLACED by their position-ordered forms.  Out of memory
// leaves the problem on the row-major form, which needs none of this.  Ends with the stream waited for: L dies with the caller's scope.
void upload_colsort(gsfm_rot_problem* P, ColsortHost& L, hvec<uint32_t>& col, hvec<uint32_t>& deid) {
  auto& C = P->cs;
  const hipStream_t s = P->stream;
  C.nch = L.nch; C.n_wg = (uint32_t)L.wg.size(); C.n_pos = L.n_pos; C.cbits = L.cbits; C.cmax = L.cmax;
  // The 2-byte record pays where an escape (a step of 15 cameras or more, a row with 7 or more entries in one sub-chunk: each its own 32-byte
  // sector) is rare: below one position in a hundred -- the benchmark graph has 1e-4 --; an allocation that fails leaves the 4-byte record in use.
  if (L.k16_mode != 0 && (L.k16_mode > 0 || (double)L.k16_escapes <= 0.01 * (double)L.n_pos)) {
    if (C.k16.upload(L.k16, s) == hipSuccess && C.kbase.upload(L.kbase, s) == hipSuccess && C.kdel.upload(L.kdel, s) == hipSuccess) C.k16_active = true;
    else { (void)hipGetLastError(); C.k16.release(); C.kbase.release(); C.kdel.release(); }
  }
  const bool up = C.wg.upload(L.wg, s) == hipSuccess && C.meta.upload(L.meta, s) == hipSuccess && (C.k16_active || C.kcol.upload(L.kcol, s) == hipSuccess) &&
                  C.kcnt.upload(L.kcnt, s) == hipSuccess && C.part.alloc((size_t)9 * C.n_wg * GSFM_COL_RB) == hipSuccess;
  if (sync_stream(s, "uploading the column-sorted layout") != 0 || !up) {
    (void)hipGetLastError();
    C = gsfm_rot_problem::ColSort();
    return;
  }
  if (getenv("GSFM_CREATE_TIMING")) fprintf(stderr, "gsfm create: column-sorted layout, %zu positions, 2-byte record %s (%llu escapes)\n", L.n_pos, C.k16_active ? "on" : "off", (unsigned long long)L.k16_escapes);
  col.swap(L.col); deid.swap(L.eid);
  C.active = true;
}

// K2c / K3c, the column-sorted layout of the directed entries: for large graphs whose rows offer the gathers no locality -- i.e. where
// neither the relabelling nor the two-level preconditioner (both for spatially coherent graphs) applies.  GSFM_K3_COLSORT=0/1 overrides.
void choose_colsort(gsfm_rot_problem* P, HostStructure& H, int n_threads) {
  const char* env = getenv("GSFM_K3_COLSORT");
  const int mode = env && *env ? atoi(env) : -1;
  const size_t nd = H.nd();
  // ROUND 6: no density condition any more.  Rounds 3-5 also asked for 512 rows x mean degree >= cameras / 2 ("sparser blocks gain nothing": the
  // gathers of a block then share no lines) -- a rule set when the layout was first built and never re-measured.  Measured on the current kernels
  // (tools/r06_density_probe.py, profiles/r06_density_rule.txt; same generator, default choice against the forced layout, whole solves):
  //   400k cameras / 40 M edges   86.8 -> 52.1 ms   (mat-vec 19.2 -> 9.2 ns per 1000 directed entries; C5: 9.35)
  //   800k / 80 M                198.2 -> 121.7 ms   (22.5 -> 11.7)        1.5 M / 150 M   423.8 -> 245.1 ms   (24.3 -> 11.4)
  //   1 M / 10 M (degree 20)     376 -> 244 ms       500k / 12.5 M (degree 50)   51.1 -> 32.8 ms     2 M / 10 M (degree 10)   12.6 -> 9.5 s
  // with the final cost equal to the last bit every time.  (Why the sorted order wins even where a wavefront's 64 gathers touch 64 different
  // lines was not chased with counters: those lines are neighbours in memory, a row-major row's are scattered over the whole vector.)
  // What remains of the rule: at least 1 M directed entries (below, the launch-latency regime, the row-major
  // kernels with their 2-kernel PCG iteration are the faster ones) and no locality found by the relabelling / no coarse space (coherent graphs).
  if (!(P->lap_capable && nd > 0 && (mode > 0 || (mode < 0 && nd >= (size_t)1000000 && P->coarse_want == 0 && P->perm.empty())))) return;
  ColsortHost L;
  if (build_colsort_host(P->n_cams, P->n_rows, H.rp, H.col, H.deid, n_threads, L)) upload_colsort(P, L, H.col, H.deid);
  if (P->cs.active) { P->coarse_want = 0; P->coarse_adaptive = false; }
}

// ---- uploads: measurement planes of the cost edges and of the directed entries, cost tiles, graph structure, normal-equation blocks ----
int upload_structure(gsfm_rot_problem* P, const HostStructure& H, const double* rel_aa, size_t nd_planes) {
  {
    DevBuf<double> d_rel;   // the measurements go up once; both sets of planes are gathered from them on the device
    if (d_rel.alloc(3 * H.n_edges) != hipSuccess || (H.n_edges > 0 && hipMemcpyAsync(d_rel.p, rel_aa, 24 * H.n_edges, hipMemcpyHostToDevice, P->stream) != hipSuccess))
      return fail(GSFM_ERR_HIP, "uploading the relative rotations failed");
    if (int st = upload_planes(P, P->cost, H.cost_eid, d_rel.p)) return st;
    if (int st = upload_planes(P, P->dir, H.deid, d_rel.p)) return st;
    if (int st = sync_stream(P->stream, "building the measurement planes")) return st;   // (this phase's one wait, here because d_rel is freed here)
  }
  // (H and the caller's arrays outlive every phase: their copies are waited for at the next phase's sync, the last ones at the end of the creation)
  if (P->cost_tiles.upload(H.tiles, P->stream) != hipSuccess) return fail(GSFM_ERR_HIP, "uploading cost tiles failed");
  P->nb_cost = (int)H.tiles.size();
  if (P->cost_idx.upload(H.cidx, P->stream) != hipSuccess || P->row_ptr.upload(H.rp, P->stream) != hipSuccess || P->col.upload(H.col, P->stream) != hipSuccess)
    return fail(GSFM_ERR_HIP, "uploading graph structure failed");
  // planes h3, h4 (the last three of the nine values of a general block) are allocated on first use: the Laplacian form needs six
  if (P->h0.alloc(nd_planes) != hipSuccess || P->h1.alloc(nd_planes) != hipSuccess || P->h2.alloc(nd_planes) != hipSuccess)
    return fail(GSFM_ERR_HIP, "allocating normal-equation blocks failed");
  return 0;
}

// K0 whitening, straight from the caller's arrays (no staging copy: cov6 is 48 B per edge)
int whiten_planes(gsfm_rot_problem* P, uint64_t n_edges, const double* cov6, const double* inlier_weight) {
  if (P->wmode == W_NONE) return 0;
  const ErrorTypeInfo et = classify_error_type(P->error_type);
  DevBuf<double> d_cov, d_inl;
  if (cov6 && et.need_cov && (d_cov.alloc(6 * n_edges) != hipSuccess || (n_edges && hipMemcpyAsync(d_cov.p, cov6, 48 * n_edges, hipMemcpyHostToDevice, P->stream) != hipSuccess)))
    return fail(GSFM_ERR_HIP, "upload cov6");
  if (inlier_weight && et.need_inl && (d_inl.alloc(n_edges) != hipSuccess || (n_edges && hipMemcpyAsync(d_inl.p, inlier_weight, 8 * n_edges, hipMemcpyHostToDevice, P->stream) != hipSuccess)))
    return fail(GSFM_ERR_HIP, "upload inlier weights");
  run_whiten(P, P->cost, d_cov.p, d_inl.p);
  run_whiten(P, P->dir, d_cov.p, d_inl.p);
  return sync_stream(P->stream, "whitening");   // (d_cov, d_inl are freed here)
}

// ---- camera buffers, and the launch geometry that sizes some of them ----
int alloc_camera_buffers(gsfm_rot_problem* P) {
  const size_t N = P->n_cams, NP = P->n_pad;
  P->nb_cam = grid_for(N);
  if (P->nb_cam > GSFM_MAX_PARTIALS * 64) return fail(GSFM_ERR_INVALID_ARG, "too many cameras");
  {  // fused mat-vec of the single-reduction PCG: one row group (256 / G rows) per workgroup unless that leaves too many partials
    const size_t rows_per_group = GSFM_BLOCK / P->G, groups = (P->n_rows + rows_per_group - 1) / rows_per_group;
    size_t max_partials = GSFM_MV_MAX_PARTIALS;
    if (P->sharded) {   // the delta partials travel in the tail of the all-gather slot: the same, rank-independent bound on every rank
      P->w_tail = 8u * (uint32_t)grid_for(P->shard.slice_width);
      max_partials = std::min<size_t>(max_partials, P->w_tail);
    }
    P->mv_reps = (int)std::max<size_t>(1, (groups + max_partials - 1) / max_partials);
    P->nb_mv = (int)std::max<size_t>(1, (groups + P->mv_reps - 1) / P->mv_reps);
  }
  bool ok = true;
  auto plain = [&](auto& buf, size_t count) { ok = ok && buf.alloc(count) == hipSuccess; };
  auto zeroed = [&](auto& buf, size_t count) { ok = ok && buf.alloc_zeroed(count, P->stream) == hipSuccess; };
  const size_t nb = (size_t)P->nb_cam;
  zeroed(P->x, 4 * N); zeroed(P->x_trial, 4 * N); zeroed(P->aa_io, 3 * N); zeroed(P->active, NP); zeroed(P->scale, 3 * N); zeroed(P->gD, 9 * NP);
  plain(P->Mblk, 6 * N); plain(P->Minv, 6 * N); plain(P->Lam, 6 * N); plain(P->Tinv, 9 * N); plain(P->b, 3 * N); plain(P->D6, 6 * N);
  plain(P->q, 2 * N); plain(P->q_trial, 2 * N);
  zeroed(P->xcg, 3 * NP); zeroed(P->r, 3 * NP); plain(P->z, 3 * N);   // (xcg, r: padded like p / Ap -- a packed sharded problem all-gathers them)
  zeroed(P->p, 3 * NP); zeroed(P->Ap, 3 * NP); zeroed(P->u_rot, 3 * NP);
  plain(P->part_a, nb); plain(P->part_b, nb); plain(P->part_cam, 6 * nb); plain(P->part_gauge, 9 * nb); plain(P->part_cost, (size_t)2 * P->nb_cost);
  zeroed(P->scal, SC_ALL); zeroed(P->cgsc, 1);
  zeroed(P->s_dir, 3 * N); zeroed(P->part_g2, 2 * nb); zeroed(P->part_d2, std::max(P->nb_mv, P->nb_cam)); zeroed(P->cg2sc, 1);
  // (here, not at the first solve: an allocation that fails on one rank only must be part of the create-time agreement)
  if (P->sharded) zeroed(P->w_gather, ((size_t)3 * P->shard.slice_width + P->w_tail) * P->shard.world_size);
  return ok ? 0 : fail(GSFM_ERR_HIP, "allocating camera buffers failed");
}

// cameras touched by at least one edge (Ceres only knows parameter blocks that appear in a residual block)
int upload_active_mask(gsfm_rot_problem* P, const std::vector<uint32_t>& rp) {
  std::vector<double> act(P->n_pad, 0.0);
  for (uint32_t r = 0; r < P->n_rows; ++r) act[P->own_begin + r] = (rp[r + 1] > rp[r]) ? 1.0 : 0.0;
  if (hipMemcpyAsync(P->active.p, act.data(), 8 * (size_t)P->n_pad, hipMemcpyHostToDevice, P->stream) != hipSuccess) return fail(GSFM_ERR_HIP, "upload active mask");
  return sync_stream(P->stream, "upload active mask");
}

// ---- sharded: the component labels, the agreement, the collectives after it ----
// connected components among this rank's own edges, as one label per camera (the smallest camera index of its component; untouched
// cameras label themselves), in this rank's slot of d_labels: merged across the ranks by sharded_agreement
int local_component_labels(gsfm_rot_problem* P, const HostStructure& H, std::vector<uint32_t>* comp_label, DevBuf<double>* d_labels) {
  const uint32_t NP = P->n_pad;
  UnionFind uf(NP);
  for (uint64_t e = 0; e < H.n_edges; ++e) uf.unite(H.edge_i[e], H.edge_j[e]);
  for (uint32_t c = 0; c < NP; ++c) uf.parent[c] = uf.find(c);
  comp_label->swap(uf.parent);
  if (d_labels->alloc((size_t)P->shard.world_size * NP) != hipSuccess) return fail(GSFM_ERR_HIP, "allocating the component labels failed");
  std::vector<double> lab(NP);
  for (uint32_t c = 0; c < NP; ++c) lab[c] = (double)(*comp_label)[c];
  if (hipMemcpyAsync(d_labels->p + (size_t)P->shard.rank * NP, lab.data(), 8 * (size_t)NP, hipMemcpyHostToDevice, P->stream) != hipSuccess) return fail(GSFM_ERR_HIP, "upload component labels");
  return sync_stream(P->stream, "upload component labels");
}

// A rank of a sharded problem sees only its own edges, so whether the GLOBAL view graph is connected -- which decides the PCG tolerance,
// see lm_solve -- is worked out from every rank's local components (union of "c and its local label are connected" over all
// ranks), identically on every rank.  (Round 2 relied on a flag the partitioner had to set; a raw C-ABI user who forgot it got a looser
// solve than on one GPU.  The flag is still honoured.)  all: every rank's labels, rank by rank; act: the gathered active mask.
uint32_t global_component_count(const std::vector<double>& all, const std::vector<double>& act, uint32_t NP, int world_size) {
  UnionFind uf(NP);
  for (int r = 0; r < world_size; ++r)
    for (uint32_t c = 0; c < NP; ++c) {
      const uint32_t l = (uint32_t)all[(size_t)r * NP + c];
      if (l != c && l < NP) uf.unite(c, l);
    }
  uint32_t comps = 0;
  for (uint32_t c = 0; c < NP; ++c) if (act[c] != 0.0 && uf.find(c) == c) ++comps;
  return comps;
}

// PACKED (round 5; SURVEY 8(e): "whole components can be packed per GPU => zero cross-GPU coupling except the scalar cost"): no rank holds an
// edge that leaves its own slice -- every camera a rank's edges touch, and the label they gave it, lies in that rank's slice.  Read off the
// gathered labels, so every rank arrives at the same verdict without another collective.  The normal matrix is then block diagonal ACROSS
// the ranks and each rank solves its own block with its own PCG (solver_pcg.hpp): no collective inside the PCG loop at all.
bool packed_verdict(const std::vector<double>& all, uint32_t NP, const gsfm_rot_shard& shard) {
  for (int r = 0; r < shard.world_size; ++r) {
    const uint64_t lo = std::min<uint64_t>((uint64_t)r * shard.slice_width, NP), hi = std::min<uint64_t>((uint64_t)(r + 1) * shard.slice_width, NP);
    for (uint32_t c = 0; c < NP; ++c) {
      const uint32_t l = (uint32_t)all[(size_t)r * NP + c];
      if (l != c && !(c >= lo && c < hi && l >= lo && l < hi)) return false;
    }
  }
  return true;
}

// this rank's own components of a packed problem, for the per-component step (solver_components.hpp): labels of its own cameras that carry an edge
void own_components(gsfm_rot_problem* P, const std::vector<double>& act, const std::vector<uint32_t>& comp_label) {
  auto& C = P->comps;
  C.comp_of.assign(P->n_cams, 0xffffffffu); C.size.clear();
  std::vector<uint32_t> id_of_root(P->n_pad, 0xffffffffu);
  for (uint32_t c = P->own_begin; c < P->own_end; ++c) {
    if (act[c] == 0.0) continue;
    const uint32_t r = comp_label[c];
    if (id_of_root[r] == 0xffffffffu) { id_of_root[r] = (uint32_t)C.size.size(); C.size.push_back(0); }
    C.comp_of[c] = id_of_root[r];
    C.size[id_of_root[r]]++;
  }
}

// The agreement, after ALL of this rank's local work, then collectives only: the active mask and every rank's component labels are gathered;
// from them the global component count, the packed verdict and (packed) this rank's own components.
int sharded_agreement(CreateCtx& ctx, const std::vector<uint32_t>& comp_label, DevBuf<double>& d_labels) {
  gsfm_rot_problem* P = ctx.P;
  const uint32_t NP = P->n_pad;
  // the two-level preconditioner is used only if every rank chose it (each judged the coherence of its own edges; the wait-and-see mode is single-GPU only)
  const int failed = ctx.agree(0.0, (P->coarse_want && !P->coarse_adaptive) ? 0.0 : 1.0);
  if (failed != 0) return fail(GSFM_ERR_COMM, failed > 0 ? "problem creation failed on " + std::to_string(failed) + " other rank(s)" : std::string("the create-time agreement all-reduce failed"));
  if (ctx.coarse_votes_against > 0.5) P->coarse_want = 0;
  if (int st = all_gather(P, P->active.p, P->shard.slice_width)) return st;
  if (int st = all_gather(P, d_labels.p, NP)) return st;
  std::vector<double> all((size_t)P->shard.world_size * NP), act(NP);
  if (int st = read_back(P, all.data(), d_labels.p, 8 * all.size(), "active mask / component labels all-gather")) return st;
  if (int st = read_back(P, act.data(), P->active.p, 8 * (size_t)NP, "download active mask")) return st;
  const uint32_t comps = global_component_count(all, act, NP, P->shard.world_size);
  P->n_components = std::max<uint32_t>(std::max<uint32_t>(1, comps), (P->shard.flags & GSFM_SHARD_DISCONNECTED) ? 2u : 1u);
  P->packed = P->n_components > 1 && packed_verdict(all, NP, P->shard);
  if (P->packed) {
    own_components(P, act, comp_label);
    P->coarse_want = 0;   // (its coarse matrix is an all-reduce per LM step and its use a decision taken from the iteration counts, which now differ from rank to rank)
  }
  return 0;
}

// The spare set of the fused trial evaluation (solver_lm.hpp, evaluate_trial): one GPU, column-sorted layout, the instantiations that have
// the fused kernel -- and only if it leaves GSFM_TRIAL_LIN_RESERVE_MB (default 4096) of the device's memory free; otherwise every trial
// point is evaluated by K1, as before.  At C5 it is 0.96 GB.
void alloc_trial_spare_set(gsfm_rot_problem* P, size_t nd_planes) {
  const int w = (P->wmode == W_MATRIX && P->q3) ? W_MATRIX3 : P->wmode;
  if (P->sharded || !P->cs.active || !col_lin_cost_kernel(P->functor, w, LM_MAGSAC)) return;
  const char* e = getenv("GSFM_TRIAL_LIN_RESERVE_MB");
  const double reserve = (e && *e ? atof(e) : 4096.0) * 1048576.0;
  const size_t NP = P->n_pad, need = 3 * sizeof(double2) * nd_planes + 8 * (9 * NP + (size_t)P->cs.n_wg);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b >= (double)need + reserve) {
    if (P->h0_b.alloc(nd_planes) != hipSuccess || P->h1_b.alloc(nd_planes) != hipSuccess || P->h2_b.alloc(nd_planes) != hipSuccess ||
        P->gD_b.alloc_zeroed(9 * NP, P->stream) != hipSuccess || P->cs.cost_part.alloc(P->cs.n_wg) != hipSuccess) {
      P->h0_b.release(); P->h1_b.release(); P->h2_b.release(); P->gD_b.release(); P->cs.cost_part.release();
    }
  }
  (void)hipGetLastError();
}

static gsfm_status problem_create_impl(uint32_t n_cams, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j,
                                       const double* rel_aa, int32_t error_type, const double* cov6, const double* inlier_weight,
                                       const gsfm_rot_shard* shard, gsfm_rot_problem** out, gsfm_rot_problem** live) {
  if (!out) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  // (one rank of a sharded problem may hold no edge at all -- a slice of isolated cameras -- and still takes part in every collective)
  const bool multi_rank = shard && (shard->world_size > 1 || (shard->world_size == 1 && getenv("GSFM_FORCE_SHARD")));
  // Two failures cannot be agreed about with the other ranks and return at once: a descriptor without callbacks (there is nothing to call)
  // and a process without a HIP device (the callbacks take device pointers).  Everything else below goes through bail().
  if (multi_rank && (!shard->all_gather || !shard->all_reduce_sum)) return (gsfm_status)fail(GSFM_ERR_INVALID_ARG, "bad shard descriptor: missing collective callbacks");
  if (const char* why = no_device_reason("the rotation solver")) return (gsfm_status)fail(GSFM_ERR_NO_DEVICE, why);

  gsfm_rot_problem* P = new gsfm_rot_problem;
  *live = P;
  CreateCtx ctx(P, live);
  if (int st = open_problem(P, shard, multi_rank)) return ctx.bail(st);
  if (int st = set_problem_fields(P, n_cams, n_edges, edge_i, edge_j, rel_aa, error_type, cov6, inlier_weight, shard, multi_rank)) return ctx.bail(st);

  // ---- host-side structure ----
  HostStructure H = host_structure_input(P, n_edges, edge_i, edge_j);
  const int n_threads = host_threads();
  if (int st = build_rows(H, n_threads)) return ctx.bail(st);
  ctx.lap("directed rows (CSR)");
  if (int st = relabel_rows(H, &P->perm, n_threads)) return ctx.bail(st);
  ctx.lap("locality relabelling");
  choose_coarse_space(P, H);
  components_on_one_gpu(P, H);
  ctx.lap("connected components");
  const size_t nd = H.nd();
  P->G = row_lanes(P->n_rows, nd);
  P->cost_direct = build_cost_tiles(H, n_threads);
  P->h_cost_eid = H.cost_eid;
  ctx.lap("cost tiles");
  P->timer.apply_rule(nd);
  P->q3 = three_component_planes(P->wmode, n_edges);
  choose_colsort(P, H, n_threads);
  ctx.lap("column-sorted layout");
  const size_t nd_planes = P->cs.active ? P->cs.n_pos : nd;   // per-entry planes: one per position (padded sub-chunks) in the column-sorted layout

  // ---- device ----
  if (int st = upload_structure(P, H, rel_aa, nd_planes)) return ctx.bail(st);
  ctx.lap("edge planes -> device");
  if (int st = whiten_planes(P, n_edges, cov6, inlier_weight)) return ctx.bail(st);
  ctx.lap("whitening");
  if (int st = alloc_camera_buffers(P)) return ctx.bail(st);
  if (int st = upload_active_mask(P, H.rp)) return ctx.bail(st);
  if (int st = prepare_loss(P, nullptr, 0)) return ctx.bail(st);
  std::vector<uint32_t> comp_label;
  DevBuf<double> d_labels;
  if (P->sharded) if (int st = local_component_labels(P, H, &comp_label, &d_labels)) return ctx.bail(st);
  ctx.lap("camera buffers");
  if (P->sharded) if (int st = sharded_agreement(ctx, comp_label, d_labels)) return ctx.bail(st);
  alloc_trial_spare_set(P, nd_planes);
  if (int st = sync_stream(P->stream, "problem creation")) return ctx.bail(st);   // (the clears and the last copies: gsfm_rot_set_stream may follow at once)
  *live = nullptr;
  *out = P;
  return GSFM_OK;
}

}  // namespace
