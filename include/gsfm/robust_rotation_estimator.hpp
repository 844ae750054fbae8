// theia::RobustRotationEstimator with Theia's public surface (sfm/global_pose_estimation/robust_rotation_estimator.h): the L1 + IRLS
// method of Chatterjee and Govindu, Theia's ROBUST_L1L2, implemented on the MI355X through the C-ABI of include/gsfm_rot_l1l2.h, which
// carries the definition.
#pragma once
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "compat.hpp"
#include "../gsfm_rot_l1l2.h"

namespace theia {

class RobustRotationEstimator : public RotationEstimator {
 public:
  struct Options {
    // Theia's field names and defaults; what each one decides is written out in include/gsfm_rot_l1l2.h
    int max_num_l1_iterations = 5;                    // outer iterations of the L1 stage
    double l1_step_convergence_threshold = 0.001;     // the L1 stage ends once the mean step is at or below this
    int max_num_irls_iterations = 100;
    double irls_step_convergence_threshold = 0.001;   // the IRLS stage ends once the mean step is below this
    double irls_loss_parameter_sigma = 5.0 * 3.14159265358979323846 / 180.0;   // sigma of the IRLS weight, radians
  };

  explicit RobustRotationEstimator(const Options& options) : options_(options) {}
  RobustRotationEstimator() {}

  // (1) the plugin entry point of theia::RotationEstimator.  In / out: orientations (start -> estimate).  The view pairs are added in
  //     ViewIdPair order (the reference: hash order), behind whatever AddRelativeRotationConstraint added before.
  bool EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) override;

  // (2) constraints one at a time -- a pair may be added more than once, each listing is an edge of its own -- then the solve.  Edges go
  //     to the device in the order they were added.  A constraint whose views have no orientation is refused by the solve (the
  //     reference's FindOrDie aborts).
  void AddRelativeRotationConstraint(const ViewIdPair& view_id_pair, const Eigen::Vector3d& relative_rotation);
  bool EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations);

  // ---- additions of this build (absent from the reference) ----
  // The view held constant by the last call: global_orientations->begin(), as GSfMNonlinearPositionEstimator chooses its fixed camera
  // (the reference's view_id_to_index_ gives that view the index -1).  kInvalidViewId before a call got that far.
  ViewId FixedView() const { return fixed_view_; }
  const gsfm_rot_l1l2_summary& LastSummary() const { return summary_; }
  const char* LastError() const { return error_.c_str(); }
  // the linear-solver and ADMM options of include/gsfm_rot_l1l2.h; the five fields of Options above are overwritten from options_ at every call
  gsfm_rot_l1l2_options* MutableSolverOptions() { return &solver_options(); }

 private:
  gsfm_rot_l1l2_options& solver_options() { if (!solver_set_) { gsfm_rot_l1l2_options_default(&solver_); solver_set_ = true; } return solver_; }

  Options options_;
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> relative_rotations_;
  ViewId fixed_view_ = kInvalidViewId;
  gsfm_rot_l1l2_summary summary_{};
  gsfm_rot_l1l2_options solver_{};
  bool solver_set_ = false;
  std::string error_;
};

}  // namespace theia
