// The front end of the entries over cameras and a track CSR (track_ptr, obs_cam, obs_xy): both triangulation entries (triangulate.hpp, track_refine.hpp),
// gsfm_tracks_outlier_tracks (outlier_tracks.hpp), gsfm_tracks_select_good (track_select.hpp), gsfm_tracks_launch_order (gsfm_rot.hip), the creation of both bundle problems (solver_ba.hpp, solver_full_ba.hpp).
// Plain C++ first (tests/cpp/track_scene_test.cpp builds it with the host compiler alone): lane classes, launch order, the checks of the track arrays.  Under
// hipcc: the scene in a one-shot call's slab (TrackScene), the launcher over the lane classes, the one-leaf loss of the three reprojection solvers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

namespace {

constexpr uint64_t TRI_LEN_G4 = 8, TRI_LEN_G16 = 64;   // triangulate_kernels.hpp's GSFM_TRI_LEN_G4 / GSFM_TRI_LEN_G16 (asserted below)
// 0, 1, 2: groups of 4, 16, 64 lanes -- a function of the track's length alone (include/gsfm_tracks.h)
inline int tri_class_of(uint64_t len) { return len <= TRI_LEN_G4 ? 0 : len <= TRI_LEN_G16 ? 1 : 2; }

// The launch order: the tracks of class 0, then 1, then 2; inside a class by descending length, equal lengths by track index.
// class_begin[c] .. class_begin[c + 1] is class c's slice of `order`.
inline void tri_bucket(uint64_t n_tracks, const uint64_t* track_ptr, uint32_t* order, uint64_t class_begin[4]) {
  uint64_t count[3] = {0, 0, 0};
  for (uint64_t t = 0; t < n_tracks; ++t) ++count[tri_class_of(track_ptr[t + 1] - track_ptr[t])];
  class_begin[0] = 0;
  for (int c = 0; c < 3; ++c) class_begin[c + 1] = class_begin[c] + count[c];
  uint64_t cursor[3] = {class_begin[0], class_begin[1], class_begin[2]};
  for (uint64_t t = 0; t < n_tracks; ++t) order[cursor[tri_class_of(track_ptr[t + 1] - track_ptr[t])]++] = (uint32_t)t;
  for (int c = 0; c < 3; ++c)
    std::stable_sort(order + class_begin[c], order + class_begin[c + 1], [track_ptr](uint32_t x, uint32_t y) {
      return track_ptr[x + 1] - track_ptr[x] > track_ptr[y + 1] - track_ptr[y];
    });
}
// tri_bucket's order (slices `all`) without the tracks whose flag is 0 (NULL flags: none), in place, the class slices kept; returns what is left
inline uint64_t tri_keep_estimated(uint32_t* order, const uint64_t all[4], const uint8_t* point_estimated, uint64_t class_begin[4]) {
  uint64_t n = class_begin[0] = 0;
  for (int c = 0; c < 3; ++c) {
    for (uint64_t k = all[c]; k < all[c + 1]; ++k) if (!point_estimated || point_estimated[order[k]]) order[n++] = order[k];
    class_begin[c + 1] = n;
  }
  return n;
}

// an entry refuses 2^31 tracks (the launch order), that or a track of 2^31 observations (the one-shot calls), or 2^31 observations or cam_nodes + n_tracks nodes (BA)
enum class TrackLimit { tracks, tracks_and_lengths, observations_and_nodes };

// The checks of track_ptr in the order every entry reports them: NULL (null_message; NULL: the caller has looked), 2^31 tracks before anything is
// read, track_ptr[0] where first_is_zero asks for it, track by track a decrease or a track too long, then the bundle adjustments' size.  false: *why
inline bool track_ptr_ok(uint64_t n_tracks, const uint64_t* track_ptr, TrackLimit limit, uint64_t cam_nodes, bool first_is_zero, const char* null_message, std::string* why) {
  const uint64_t big = 1ull << 31;
  auto refuse = [why](const std::string& message) { *why = message; return false; };
  if (null_message && !track_ptr) return refuse(null_message);
  if (limit != TrackLimit::observations_and_nodes && n_tracks >= big) return refuse("problem too large (2^31 tracks)");
  if (first_is_zero && track_ptr[0] != 0) return refuse("track_ptr[0] must be 0");
  for (uint64_t t = 0; t < n_tracks; ++t) {
    if (track_ptr[t + 1] < track_ptr[t]) return refuse("track_ptr decreases at track " + std::to_string(t));
    if (limit == TrackLimit::tracks_and_lengths && track_ptr[t + 1] - track_ptr[t] >= big) return refuse("track " + std::to_string(t) + " is too long (2^31 observations)");
  }
  if (limit == TrackLimit::observations_and_nodes && (track_ptr[n_tracks] >= big || cam_nodes + n_tracks >= big)) return refuse("problem too large (2^31 observations or nodes)");
  return true;
}
// the checks of the n_obs = track_ptr[n_tracks] observations, after track_ptr_ok
inline bool track_obs_ok(uint32_t n_cams, uint64_t n_obs, const uint32_t* obs_cam, const double* obs_xy, std::string* why) {
  if (n_obs > 0 && (!obs_cam || !obs_xy)) { *why = "NULL argument"; return false; }
  for (uint64_t k = 0; k < n_obs; ++k) if (obs_cam[k] >= n_cams) { *why = "observation " + std::to_string(k) + " has an out-of-range camera index"; return false; }
  return true;
}

}  // namespace

#ifdef __HIPCC__
#include <type_traits>
#include "flat_call.hpp"
#include "triangulate_kernels.hpp"
#include "../../include/gsfm_tracks.h"

namespace {
static_assert(TRI_LEN_G4 == GSFM_TRI_LEN_G4 && TRI_LEN_G16 == GSFM_TRI_LEN_G16, "the host's lane classes are not the kernels'");

// a bound of the gate: 0, or the refusal of a value that is negative or not finite
int gate_bound_check(double v, const char* name) { return v >= 0.0 && std::isfinite(v) ? 0 : fail(GSFM_ERR_INVALID_ARG, std::string(name) + " must be finite and not negative"); }
// both checks of the track arrays for an entry: 0, or GSFM_ERR_INVALID_ARG with the message set
int track_arrays_check(uint32_t n_cams, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, TrackLimit limit, uint64_t cam_nodes,
                       const char* null_message) {
  std::string why;
  if (track_ptr_ok(n_tracks, track_ptr, limit, cam_nodes, true, null_message, &why) && track_obs_ok(n_cams, track_ptr[n_tracks], obs_cam, obs_xy, &why)) return 0;
  return fail(GSFM_ERR_INVALID_ARG, why);
}

// fn(G, n_slots, offset, grid, block) for the lane classes of G = 64, 16, 4 lanes (a compile-time constant: the kernels are templates over it) that have
// tracks, the long tracks first: cb is the launch order's class slices, a group of 64 lanes is a block, GSFM_TRI_BLOCK lanes hold the smaller groups
template <typename Fn> void for_lane_classes(const uint64_t cb[4], Fn fn) {
  auto grid = [](uint64_t n_slots, unsigned groups_per_block) { return dim3((unsigned)((n_slots + groups_per_block - 1) / groups_per_block)); };
  if (cb[3] > cb[2]) fn(std::integral_constant<int, 64>(), cb[3] - cb[2], cb[2], grid(cb[3] - cb[2], 1), dim3(64));
  if (cb[2] > cb[1]) fn(std::integral_constant<int, 16>(), cb[2] - cb[1], cb[1], grid(cb[2] - cb[1], GSFM_TRI_BLOCK / 16), dim3(GSFM_TRI_BLOCK));
  if (cb[1] > cb[0]) fn(std::integral_constant<int, 4>(), cb[1] - cb[0], cb[0], grid(cb[1] - cb[0], GSFM_TRI_BLOCK / 4), dim3(GSFM_TRI_BLOCK));
}

// The scene of a one-shot call in its slab: the launch order (n_order entries), the track CSR, the cameras as given and as k_tri_cameras' records, the
// plane scratch of the 64-lane class, the per-track results
struct TrackScene {
  size_t n_order = 0, T = 0, N = 0, O = 0;
  Slot<uint32_t> s_ord, s_cam; Slot<uint64_t> s_ptr; Slot<double2> s_xy; Slot<uint8_t> s_est; Slot<int32_t> s_st, s_nv;
  Slot<double> s_rot, s_pos, s_k, s_rec, s_plane, s_pt, s_err;
  void take(FlatLayout& L, size_t n_order_, size_t n_tracks, size_t n_cams, size_t n_obs, bool long_class) {
    n_order = n_order_; T = n_tracks; N = n_cams; O = n_obs;
    s_ord = L.take<uint32_t>(n_order); s_ptr = L.take<uint64_t>(T + 1); s_cam = L.take<uint32_t>(O); s_xy = L.take<double2>(O);
    s_rot = L.take<double>(3 * N); s_pos = L.take<double>(3 * N); s_k = L.take<double>(3 * N); s_est = L.take<uint8_t>(N);
    s_rec = L.take<double>(GSFM_TRI_CAM_DOUBLES * N); s_plane = L.take<double>(long_class ? 3 * O : 0); s_pt = L.take<double>(3 * T);
    s_st = L.take<int32_t>(T); s_nv = L.take<int32_t>(T); s_err = L.take<double>(T);
  }
  // 0, or the status of a failed copy (the message is set)
  int upload(FlatCall& fc, const uint32_t* order, const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const double* rot_aa, const double* cam_pos,
             const double* intrinsics, const uint8_t* cam_estimated) const {
    HIPCHK(fc.upload(s_ord, order, n_order)); HIPCHK(fc.upload(s_ptr, track_ptr, T + 1));
    if (O > 0) { HIPCHK(fc.upload(s_cam, obs_cam, O)); HIPCHK(fc.upload(s_xy, obs_xy, O)); }
    if (N > 0) { HIPCHK(fc.upload(s_rot, rot_aa, 3 * N)); HIPCHK(fc.upload(s_pos, cam_pos, 3 * N)); HIPCHK(fc.upload(s_k, intrinsics, 3 * N)); }
    if (N > 0 && cam_estimated) HIPCHK(fc.upload(s_est, cam_estimated, N));
    return 0;
  }
  // The camera records enqueued (estimated: whether upload() had flags; none: every camera is estimated), and the kernel arguments but the class's slice
  void start(const FlatCall& fc, bool estimated, double min_triangulation_angle_degrees, double max_reprojection_error_pixels, TriArgs* a) const {
    if (N > 0)
      hipLaunchKernelGGL(k_tri_cameras, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, fc.s, (uint32_t)N, (const double*)fc.ptr(s_rot), (const double*)fc.ptr(s_pos),
                         (const double*)fc.ptr(s_k), estimated ? (const uint8_t*)fc.ptr(s_est) : (const uint8_t*)nullptr, fc.ptr(s_rec));
    a->track_ptr = fc.ptr(s_ptr); a->obs_cam = fc.ptr(s_cam); a->obs_xy = fc.ptr(s_xy); a->cams = fc.ptr(s_rec); a->plane = fc.ptr(s_plane); a->n_obs = O;
    a->cos_min_angle = std::cos(min_triangulation_angle_degrees * M_PI / 180.0); a->max_sq_err = max_reprojection_error_pixels * max_reprojection_error_pixels;
    a->point = fc.ptr(s_pt); a->status = fc.ptr(s_st); a->n_views = fc.ptr(s_nv); a->mean_sq_err = fc.ptr(s_err);
  }
};

// The loss of a reprojection solver: nothing (Ceres' NULL loss) or ONE leaf that the kernels' loss_leaf_simple evaluates, validated without a problem (the
// ABI tests hand the bundle adjustments a handle that is no problem at all: their callers store *leaf after every refusal, and have refused a NULL program
// before; the refinement reports its node count before a NULL program).  who: "track refinement", "bundle adjustment" or "full bundle adjustment"
int one_leaf_loss(const gsfm_loss_node* prog, int32_t n, const std::string& who, gsfm::DevLossNode* leaf) {
  if (n < 0 || n > 1) return fail(GSFM_ERR_INVALID_ARG, "the " + who + " takes a loss of one leaf (composite programs are not supported)");
  if (n == 1 && !prog) return fail(GSFM_ERR_INVALID_ARG, "NULL argument");
  std::memset(leaf, 0, sizeof(*leaf));
  leaf->kind = GSFM_LOSS_TRIVIAL;
  if (n == 1) {
    const int k = prog[0].kind;
    if (!(k == GSFM_LOSS_TRIVIAL || k == GSFM_LOSS_HUBER || k == GSFM_LOSS_SOFT_L1 || k == GSFM_LOSS_TUKEY || k == GSFM_LOSS_GEMAN_MCCLURE))
      return fail(GSFM_ERR_INVALID_ARG, "the " + who + " takes the losses Trivial, Huber, SoftLOne, Tukey and GemanMcClure (MAGSAC and the other leaves are not supported)");
    for (int j = 0; j < 3; ++j) {
      if (!std::isfinite(prog[0].p[j])) return fail(GSFM_ERR_INVALID_ARG, "loss parameter is not finite");
      leaf->p[j] = prog[0].p[j];
    }
    if (k != GSFM_LOSS_TRIVIAL && !(prog[0].p[0] > 0.0)) return fail(GSFM_ERR_INVALID_ARG, "the loss width must be positive");
    leaf->kind = k;
  }
  return 0;
}

}  // namespace
#endif
