// theia::RobustRotationEstimator on the MI355X solver (include/gsfm_rot_l1l2.h).
//
// A call flattens the caller's maps into the arrays of the C-ABI -- dense camera index = rank of the ViewId among the views that have
// an orientation, edges in the order they were added -- solves on the device and writes the rotations back into the caller's map in place.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/gsfm/robust_rotation_estimator.hpp"

namespace theia {

bool RobustRotationEstimator::EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  // sorted by ViewIdPair, so that the result does not depend on the iteration order of the map
  std::vector<ViewIdPair> keys;
  keys.reserve(view_pairs.size());
  for (const auto& kv : view_pairs) keys.push_back(kv.first);
  std::sort(keys.begin(), keys.end());
  for (const ViewIdPair& k : keys) AddRelativeRotationConstraint(k, view_pairs.at(k).rotation_2);
  return EstimateRotations(global_orientations);
}

void RobustRotationEstimator::AddRelativeRotationConstraint(const ViewIdPair& view_id_pair, const Eigen::Vector3d& relative_rotation) {
  relative_rotations_.emplace_back(view_id_pair, relative_rotation);
}

bool RobustRotationEstimator::EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  error_.clear();
  std::memset(&summary_, 0, sizeof(summary_));
  fixed_view_ = kInvalidViewId;
  if (global_orientations == nullptr) { error_ = "global_orientations is NULL"; return false; }
  if (relative_rotations_.empty()) { error_ = "no relative rotation constraints were added"; return false; }   // (the reference: CHECK_GT aborts)
  if (global_orientations->empty()) { error_ = "no initial orientations were provided"; return false; }

  std::vector<ViewId> ids;
  ids.reserve(global_orientations->size());
  for (const auto& kv : *global_orientations) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  std::unordered_map<ViewId, uint32_t> index;
  index.reserve(ids.size() * 2);
  for (size_t k = 0; k < ids.size(); ++k) index[ids[k]] = (uint32_t)k;

  const size_t E = relative_rotations_.size(), N = ids.size();
  std::vector<uint32_t> ei(E), ej(E);
  std::vector<double> rel(3 * E), rot(3 * N);
  for (size_t e = 0; e < E; ++e) {
    const ViewIdPair& pair = relative_rotations_[e].first;
    const auto a = index.find(pair.first), b = index.find(pair.second);
    if (a == index.end() || b == index.end()) {
      error_ = "constraint " + std::to_string(e) + " names a view without an initial orientation";
      return false;
    }
    ei[e] = a->second; ej[e] = b->second;
    for (int c = 0; c < 3; ++c) rel[3 * e + c] = relative_rotations_[e].second[c];
  }
  for (size_t k = 0; k < N; ++k) {
    const Eigen::Vector3d& w = global_orientations->at(ids[k]);
    rot[3 * k] = w[0]; rot[3 * k + 1] = w[1]; rot[3 * k + 2] = w[2];
  }
  fixed_view_ = global_orientations->begin()->first;

  gsfm_rot_l1l2_options o = solver_options();
  o.max_num_l1_iterations = options_.max_num_l1_iterations;
  o.l1_step_convergence_threshold = options_.l1_step_convergence_threshold;
  o.max_num_irls_iterations = options_.max_num_irls_iterations;
  o.irls_step_convergence_threshold = options_.irls_step_convergence_threshold;
  o.irls_loss_parameter_sigma = options_.irls_loss_parameter_sigma;
  const gsfm_status st = gsfm_rot_l1l2_solve((uint32_t)N, E, ei.data(), ej.data(), rel.data(), rot.data(), (int32_t)index[fixed_view_], &o, &summary_);
  if (st != GSFM_OK) { error_ = gsfm_last_error(); return false; }
  for (size_t k = 0; k < N; ++k) {
    Eigen::Vector3d& w = (*global_orientations)[ids[k]];
    w[0] = rot[3 * k]; w[1] = rot[3 * k + 1]; w[2] = rot[3 * k + 2];
  }
  return summary_.nonfinite == 0;
}

}  // namespace theia
