// theia::GSfMNonlinearPositionEstimator with the reference's constructors and its two EstimatePositions signatures
// (reference include/GSfM_nonlinear_position_estimator.hpp, src/GSfM_nonlinear_position_estimator.cpp), implemented on the MI355X
// solver through the C-ABI of include/gsfm_pos.h (camera-to-camera BASELINE constraints) and, with min_num_points_per_view > 0,
// of include/gsfm_posp.h (point-to-camera constraints over the reconstruction's tracks) instead of Ceres.
#pragma once
#include <string>
#include <unordered_map>

#include "compat.hpp"
#include "../gsfm_pos.h"
#include "../gsfm_posp.h"

namespace theia {

// The reference's enum.  Both of its EstimatePositions overloads add BASELINE constraints whatever the type says (they call the
// two-argument AddCameraToCameraConstraints), so the type is accepted and has no effect here either; the Python module binds BASELINE only.
enum class PositionErrorType { BASELINE = 0, COVARIANCE = 1 };

class GSfMNonlinearPositionEstimator {
 public:
  // the fields of Theia's NonlinearPositionEstimator::Options this path reads
  struct Options {
    int num_threads = 1;                 // accepted for signature parity
    int max_num_iterations = 400;
    double robust_loss_width = 0.1;      // HuberLoss of the overload without a loss
    int min_num_points_per_view = 0;     // > 0: every view is tied to at least this many tracks (include/gsfm/position_track_selection.hpp)
    double point_to_camera_weight = 0.5; // Theia's default; must be positive.  The problem's weight is this times
                                         // (camera-to-camera residuals) / (point-to-camera constraints)
    // An addition of this build.  false (default): a feature's ray is rotated by the orientation passed to EstimatePositions, which is
    // what the reference's comment says ("rotate the feature ray to be in the global orientation frame").  true: by the orientation
    // the reconstruction stores for the view (zero when it stores none), which is what the reference and Theia 0.7 actually do: their
    // GetRotatedFeatureRay calls camera.PixelToUnitDepthRay on the reconstruction's camera and never uses the copy that received the
    // orientation argument.  The two agree whenever the caller stored the estimated orientations first (SetOrientations).
    bool rays_from_reconstruction_orientation = false;
  };

  GSfMNonlinearPositionEstimator() {}
  explicit GSfMNonlinearPositionEstimator(const Options& options) : options_(options) {}
  // the reference's constructor: the reconstruction supplies the tracks of the point-to-camera constraints (it must outlive the calls)
  GSfMNonlinearPositionEstimator(const Options& options, const Reconstruction& reconstruction) : options_(options), reconstruction_(&reconstruction) {}

  // reference .cpp:87-160: HuberLoss(robust_loss_width).  positions: every view that appears in a view pair and has an orientation
  // is set to zero (the reference's InitializeRandomPositions: its random draw is overwritten by the next line), an edge is used when
  // both of its views have a position, and positions->begin() is held constant at zero.  With min_num_points_per_view > 0 the chosen
  // tracks' points start at (1, 1, 1) (the reference's overwritten draw again) and are not returned.  Returns false for empty inputs, a
  // failed solve, a point_to_camera_weight that is not positive, min_num_points_per_view > 0 without a reconstruction, or a loss without
  // a native program on a problem with tracks (LastError()).  When no track is chosen the call is the camera-only solve.
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions);
  // reference .cpp:162-240: the caller's loss (NULL: HuberLoss(robust_loss_width)); error_type has no effect (see above)
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions, PositionErrorType error_type, ceres::LossFunction* loss_function);

  // ---- additions of this build ----
  // what the last call added of point-to-camera constraints (zeros for a camera-only solve)
  struct PointConstraints {
    uint64_t num_tracks = 0;               // chosen by the selection
    uint64_t num_constraints = 0;          // the sum of the views' credits: the reference's num_point_to_camera_constraints
    uint64_t num_observations_used = 0;    // of the solve (gsfm_posp_summary)
    uint64_t num_active_points = 0;
    double weight = 0.0;                   // the problem's w_p
  };
  const gsfm_pos_summary& LastSummary() const { return summary_; }
  const PointConstraints& LastPointConstraints() const { return points_; }
  const char* LastError() const { return error_.c_str(); }
  ViewId FixedView() const { return fixed_view_; }   // the view held constant by the last call (kInvalidViewId before one)
  gsfm_pos_options* MutableOptions() { if (!options_set_) { gsfm_pos_options_default(&solver_options_); options_set_ = true; } return &solver_options_; }
  Options* MutableEstimatorOptions() { return &options_; }

 private:
  bool Run(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs, const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
           std::unordered_map<ViewId, Eigen::Vector3d>* positions, ceres::LossFunction* loss_function);

  Options options_;
  const Reconstruction* reconstruction_ = nullptr;
  gsfm_pos_summary summary_{};
  PointConstraints points_;
  gsfm_pos_options solver_options_{};
  bool options_set_ = false;
  ViewId fixed_view_ = kInvalidViewId;
  std::string error_;
};

}  // namespace theia
