// theia::GSfMNonlinearPositionEstimator with the reference's two EstimatePositions signatures
// (reference include/GSfM_nonlinear_position_estimator.hpp, src/GSfM_nonlinear_position_estimator.cpp), implemented on the MI355X
// solver through the C-ABI of include/gsfm_pos.h instead of Ceres.  Camera-to-camera BASELINE constraints only.
#pragma once
#include <string>
#include <unordered_map>

#include "compat.hpp"
#include "../gsfm_pos.h"

namespace theia {

// The reference's enum.  Both of its EstimatePositions overloads add BASELINE constraints whatever the type says (they call the
// two-argument AddCameraToCameraConstraints), so the type is accepted and has no effect here either; the Python module binds BASELINE only.
enum class PositionErrorType { BASELINE = 0, COVARIANCE = 1 };

class GSfMNonlinearPositionEstimator {
 public:
  // the fields of Theia's NonlinearPositionEstimator::Options this path reads (point constraints are out of scope)
  struct Options {
    int num_threads = 1;                 // accepted for signature parity
    int max_num_iterations = 400;
    double robust_loss_width = 0.1;      // HuberLoss of the overload without a loss
    int min_num_points_per_view = 0;     // must stay 0: point-to-camera constraints are not implemented
  };

  GSfMNonlinearPositionEstimator() {}
  explicit GSfMNonlinearPositionEstimator(const Options& options) : options_(options) {}

  // reference .cpp:87-160: HuberLoss(robust_loss_width).  positions: every view that appears in a view pair and has an orientation
  // is set to zero (the reference's InitializeRandomPositions: its random draw is overwritten by the next line), an edge is used when
  // both of its views have a position, and positions->begin() is held constant at zero.  Returns false for empty inputs, a failed
  // solve, or a non-zero min_num_points_per_view (LastError()).
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions);
  // reference .cpp:162-240: the caller's loss (NULL: HuberLoss(robust_loss_width)); error_type has no effect (see above)
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions, PositionErrorType error_type, ceres::LossFunction* loss_function);

  // ---- additions of this build ----
  const gsfm_pos_summary& LastSummary() const { return summary_; }
  const char* LastError() const { return error_.c_str(); }
  ViewId FixedView() const { return fixed_view_; }   // the view held constant by the last call (kInvalidViewId before one)
  gsfm_pos_options* MutableOptions() { if (!options_set_) { gsfm_pos_options_default(&solver_options_); options_set_ = true; } return &solver_options_; }

 private:
  bool Run(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
           std::unordered_map<ViewId, Eigen::Vector3d>* positions, ceres::LossFunction* loss_function);

  Options options_;
  gsfm_pos_summary summary_{};
  gsfm_pos_options solver_options_{};
  bool options_set_ = false;
  ViewId fixed_view_ = kInvalidViewId;
  std::string error_;
};

}  // namespace theia
