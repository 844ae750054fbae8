// theia::GSfMNonlinearPositionEstimator on the MI355X solver (include/gsfm_pos.h; with point-to-camera constraints include/gsfm_posp.h).
//
// The positions map is built the way the reference builds it (reserve, then one assignment per view in orientations' iteration
// order), so positions->begin() -- the view the reference holds constant -- is the same view.  The solve itself sees dense camera
// indices (rank of the ViewId among the keys of *positions) and the used edges sorted by ViewIdPair, so that its result does not depend
// on unordered_map iteration order; the positions are written back in place.
//
// Point-to-camera constraints (min_num_points_per_view > 0).  The tracks come from the reconstruction's flattened tracks (FlattenTracks), chosen by
// include/gsfm/position_track_selection.hpp over the views that have a position; a chosen track's observations in views without a position are
// left out, as AddTrackToProblem skips them; the intrinsics are FlattenTracks'; every point starts at (1, 1, 1).  DEPARTURE (include/gsfm_posp.h): a
// chosen track with fewer than two observations in views with a position is no parameter.  When nothing is chosen the call is the camera-only solve.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <limits>
#include <unordered_set>
#include <vector>

#include "../../include/gsfm/GSfM_nonlinear_position_estimator.hpp"
#include "../../include/gsfm/position_track_selection.hpp"
#include "../../include/gsfm/view_graph.hpp"

namespace theia {

namespace {

struct HostLossCall {   // as in rotation_estimator.cpp: nothing may unwind through the solver's extern "C" frames
  const ceres::LossFunction* loss;
  std::exception_ptr error;
};
void host_loss_trampoline(void* user, double s, double out[3]) {
  HostLossCall* call = static_cast<HostLossCall*>(user);
  try {
    call->loss->Evaluate(s, out);
  } catch (...) {
    if (!call->error) call->error = std::current_exception();
    out[0] = out[1] = out[2] = std::numeric_limits<double>::quiet_NaN();
  }
}
struct ProblemOwner {
  gsfm_pos_problem* p = nullptr;
  ~ProblemOwner() { if (p) gsfm_pos_problem_destroy(p); }
};
struct PointProblemOwner {
  gsfm_posp_problem* p = nullptr;
  ~PointProblemOwner() { if (p) gsfm_posp_problem_destroy(p); }
};

// The arrays of gsfm_posp_problem_create beside the edges: the chosen tracks' observations in the views that have a position
struct PointArrays {
  std::vector<uint64_t> track_ptr{0};
  std::vector<uint32_t> obs_cam;
  std::vector<double> obs_xy, intrinsics, ray_rot;
  uint64_t num_constraints = 0;
};

// ids: the views that have a position, ascending (dense camera index = rank); rot: their orientations as passed to EstimatePositions
PointArrays ChoosePointConstraints(const Reconstruction& rec, const std::vector<ViewId>& ids, const std::unordered_map<ViewId, uint32_t>& index,
                                   const std::vector<double>& rot, int min_num_points_per_view, bool rays_from_reconstruction_orientation) {
  PointArrays out;
  gsfm::FlatTracks flat;
  gsfm::FlattenTracks(rec, &flat);
  const size_t T = flat.track_ptr.empty() ? 0 : flat.track_ptr.size() - 1, N = ids.size();
  if (T == 0) return out;
  std::vector<uint32_t> obs_view(flat.obs_cam.size());
  for (size_t e = 0; e < obs_view.size(); ++e) obs_view[e] = flat.views[flat.obs_cam[e]];
  const gsfm::PositionTrackSelection sel = gsfm::SelectTracksForPositionEstimation(ids, T, flat.track_ptr.data(), obs_view.data(), min_num_points_per_view);
  out.num_constraints = sel.num_point_to_camera_constraints;
  if (out.num_constraints == 0) return out;
  for (uint64_t t : sel.tracks) {
    for (uint64_t e = flat.track_ptr[t]; e < flat.track_ptr[t + 1]; ++e) {
      const auto it = index.find(obs_view[e]);
      if (it == index.end()) continue;
      out.obs_cam.push_back(it->second);
      out.obs_xy.push_back(flat.obs_xy[2 * e]); out.obs_xy.push_back(flat.obs_xy[2 * e + 1]);
    }
    out.track_ptr.push_back(out.obs_cam.size());
  }
  out.intrinsics.assign(3 * N, 0.0);
  for (size_t c = 0; c < flat.views.size(); ++c) {
    const auto it = index.find(flat.views[c]);
    if (it != index.end()) for (int k = 0; k < 3; ++k) out.intrinsics[3 * it->second + k] = flat.intrinsics[3 * c + k];
  }
  out.ray_rot = rot;
  if (rays_from_reconstruction_orientation) {
    out.ray_rot.assign(3 * N, 0.0);
    for (size_t k = 0; k < N; ++k) {
      const auto it = rec.orientation.find(ids[k]);
      if (it != rec.orientation.end()) for (int c = 0; c < 3; ++c) out.ray_rot[3 * k + c] = it->second[c];
    }
  }
  return out;
}

}  // namespace

bool GSfMNonlinearPositionEstimator::EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                       const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                       std::unordered_map<ViewId, Eigen::Vector3d>* positions) {
  return Run(view_pairs, orientations, positions, nullptr);
}

bool GSfMNonlinearPositionEstimator::EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                       const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                       std::unordered_map<ViewId, Eigen::Vector3d>* positions, PositionErrorType /*error_type*/,
                                                       ceres::LossFunction* loss_function) {
  return Run(view_pairs, orientations, positions, loss_function);
}

bool GSfMNonlinearPositionEstimator::Run(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                         const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                         std::unordered_map<ViewId, Eigen::Vector3d>* positions, ceres::LossFunction* loss_function) {
  error_.clear();
  std::memset(&summary_, 0, sizeof(summary_));
  points_ = PointConstraints();
  fixed_view_ = kInvalidViewId;
  if (positions == nullptr) { error_ = "positions is NULL"; return false; }   // CHECK_NOTNULL in the reference
  if (view_pairs.empty() || orientations.empty()) return false;
  if (options_.min_num_points_per_view < 0 || !(options_.point_to_camera_weight > 0.0)) {   // CHECK_GE / CHECK_GT in the reference's constructor
    error_ = "min_num_points_per_view must not be negative and point_to_camera_weight must be positive";
    return false;
  }
  if (options_.min_num_points_per_view > 0 && reconstruction_ == nullptr) {
    error_ = "point-to-camera constraints (min_num_points_per_view > 0) need the constructor that takes the reconstruction";
    return false;
  }

  // InitializeRandomPositions: every view of a view pair that has an orientation starts at zero
  std::unordered_set<ViewId> constrained;
  constrained.reserve(orientations.size());
  for (const auto& vp : view_pairs) { constrained.insert(vp.first.first); constrained.insert(vp.first.second); }
  positions->reserve(orientations.size());
  for (const auto& o : orientations)
    if (constrained.count(o.first)) (*positions)[o.first] = Eigen::Vector3d(0, 0, 0);
  if (positions->empty()) return false;

  // dense indices over the keys of *positions; edges whose views both have a position (and whose first view has the orientation
  // the direction is rotated by -- the reference would abort on FindOrDie there)
  std::vector<ViewId> ids;
  ids.reserve(positions->size());
  for (const auto& kv : *positions) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  std::unordered_map<ViewId, uint32_t> index;
  index.reserve(2 * ids.size());
  for (size_t k = 0; k < ids.size(); ++k) index[ids[k]] = (uint32_t)k;
  std::vector<ViewIdPair> keys;
  keys.reserve(view_pairs.size());
  for (const auto& vp : view_pairs)
    if (index.count(vp.first.first) && index.count(vp.first.second) && orientations.count(vp.first.first)) keys.push_back(vp.first);
  std::sort(keys.begin(), keys.end());
  if (keys.empty()) { error_ = "no view pair has positions at both ends"; return false; }
  const size_t N = ids.size(), E = keys.size();
  std::vector<uint32_t> ei(E), ej(E);
  std::vector<double> rel(3 * E), rot(3 * N, 0.0), pos(3 * N);
  for (size_t e = 0; e < E; ++e) {
    ei[e] = index[keys[e].first]; ej[e] = index[keys[e].second];
    const Eigen::Vector3d& t = view_pairs.at(keys[e]).position_2;
    for (int c = 0; c < 3; ++c) rel[3 * e + c] = t[c];
  }
  for (size_t k = 0; k < N; ++k) {
    auto it = orientations.find(ids[k]);
    if (it != orientations.end()) for (int c = 0; c < 3; ++c) rot[3 * k + c] = it->second[c];
  }

  // positions->begin() at zero, held constant
  fixed_view_ = positions->begin()->first;
  (*positions)[fixed_view_] = Eigen::Vector3d(0, 0, 0);
  for (size_t k = 0; k < N; ++k) { const Eigen::Vector3d& p = positions->at(ids[k]); for (int c = 0; c < 3; ++c) pos[3 * k + c] = p[c]; }
  const uint32_t fixed = index[fixed_view_];
  bool fixed_used = false;
  for (size_t e = 0; e < E && !fixed_used; ++e) fixed_used = ei[e] == fixed || ej[e] == fixed;
  if (!fixed_used) { error_ = "the view held constant (positions->begin()) is in no usable view pair"; return false; }

  if (options_.min_num_points_per_view > 0) {
    const PointArrays pts = ChoosePointConstraints(*reconstruction_, ids, index, rot, options_.min_num_points_per_view, options_.rays_from_reconstruction_orientation);
    if (pts.num_constraints > 0) {
      // the same loss for both residual kinds (AddTrackToProblem takes the loss object of the edges); a loss without a native program is refused
      gsfm_loss_node prog[GSFM_LOSS_MAX_NODES];
      int n = 1;
      std::memset(prog, 0, sizeof(prog));
      prog[0].kind = GSFM_LOSS_HUBER; prog[0].p[0] = options_.robust_loss_width;
      if (loss_function != nullptr) {
        const gsfm::DescribedLoss* d = dynamic_cast<const gsfm::DescribedLoss*>(loss_function);
        n = d ? d->NativeProgram(prog, GSFM_LOSS_MAX_NODES) : -1;
      }
      if (n < 0) { error_ = "point-to-camera constraints need a loss with a native program (a host-callback loss is not supported with tracks)"; return false; }
      const size_t T = pts.track_ptr.size() - 1;
      points_.num_tracks = T; points_.num_constraints = pts.num_constraints;
      points_.weight = gsfm::PointToCameraWeight(options_.point_to_camera_weight, E, pts.num_constraints);
      PointProblemOwner Q;
      gsfm_status st = gsfm_posp_problem_create((uint32_t)N, E, ei.data(), ej.data(), rel.data(), rot.data(), pts.ray_rot.data(), pts.intrinsics.data(), T,
                                                pts.track_ptr.data(), pts.obs_cam.data(), pts.obs_xy.data(), points_.weight, &Q.p);
      if (st == GSFM_OK) st = gsfm_posp_set_loss(Q.p, prog, n);
      if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
      gsfm_pos_options o = *MutableOptions();
      o.max_num_iterations = options_.max_num_iterations;
      std::vector<double> points(3 * T, 1.0);   // triangulated_points_[track] = (1, 1, 1)
      gsfm_posp_summary full;
      st = gsfm_posp_solve(Q.p, pos.data(), points.data(), (int32_t)fixed, &o, &full);
      if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
      summary_ = full.pos;
      points_.num_observations_used = full.num_observations_used; points_.num_active_points = full.num_active_points;
      for (size_t k = 0; k < N; ++k) (*positions)[ids[k]] = Eigen::Vector3d(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
      return summary_.termination != GSFM_TERM_FAILURE && !summary_.nonfinite;
    }
  }

  ProblemOwner P;
  gsfm_status st = gsfm_pos_problem_create((uint32_t)N, E, ei.data(), ej.data(), rel.data(), rot.data(), &P.p);
  if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
  // loss: NULL -> HuberLoss(robust_loss_width) (:294-300); a self-describing loss -> its program; anything else -> the host callback
  HostLossCall host_call{loss_function, nullptr};
  if (loss_function == nullptr) {
    gsfm_loss_node huber;
    std::memset(&huber, 0, sizeof(huber));
    huber.kind = GSFM_LOSS_HUBER; huber.p[0] = options_.robust_loss_width;
    st = gsfm_pos_set_loss(P.p, &huber, 1);
  } else {
    gsfm_loss_node prog[GSFM_LOSS_MAX_NODES];
    int n = -1;
    if (const gsfm::DescribedLoss* d = dynamic_cast<const gsfm::DescribedLoss*>(loss_function)) n = d->NativeProgram(prog, GSFM_LOSS_MAX_NODES);
    st = n >= 0 ? gsfm_pos_set_loss(P.p, prog, n) : gsfm_pos_set_loss_callback(P.p, host_loss_trampoline, &host_call);
  }
  if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
  gsfm_pos_options o = *MutableOptions();
  o.max_num_iterations = options_.max_num_iterations;
  st = gsfm_pos_solve(P.p, pos.data(), (int32_t)fixed, &o, &summary_);
  if (host_call.error) {
    gsfm_pos_problem_destroy(P.p); P.p = nullptr;
    std::rethrow_exception(host_call.error);
  }
  if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
  for (size_t k = 0; k < N; ++k) (*positions)[ids[k]] = Eigen::Vector3d(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
  // summary.IsSolutionUsable(): every termination but FAILURE
  return summary_.termination != GSFM_TERM_FAILURE && !summary_.nonfinite;
}

}  // namespace theia
