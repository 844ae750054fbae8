// pybind11 module `GlobalSfMpy`: the Python surface of the reference (bind_src/GlobalSfMpy.cpp:139-691)
// for the rotation-averaging path — everything scripts/sfm_pipeline.py touches up to its
// rotation-only exit (:31-70), the estimator classes, the loss trampoline and the gamma constants —
// backed by the MI355X solver.  Stages that are out of scope (tracks, BA, triangulation, image I/O)
// are not bound; calling them raises AttributeError instead of silently doing nothing.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <pybind11/stl_bind.h>

#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>

#include "../../include/gsfm/GSfM_nonlinear_position_estimator.hpp"
#include "../../include/gsfm/position_track_selection.hpp"
#include "../../include/gsfm/GSfM_nonlinear_rotation_estimator.hpp"
#include "../../include/gsfm/robust_rotation_estimator.hpp"
#include "../../include/gsfm/evaluation.hpp"
#include "../../include/gsfm/view_graph.hpp"
#include "../../include/gsfm_ba7.h"

namespace py = pybind11;
using namespace theia;

// numpy <-> the compat 3-vector / 3x3 (the reference relies on pybind11/eigen.h, bind :4)
namespace pybind11 { namespace detail {
template <> struct type_caster<Eigen::Vector3d> {
  PYBIND11_TYPE_CASTER(Eigen::Vector3d, _("numpy.ndarray[float64[3]]"));
  bool load(handle src, bool) {
    auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(src);
    if (!a || a.size() != 3) return false;
    for (int k = 0; k < 3; ++k) value[k] = a.data()[k];
    return true;
  }
  static handle cast(const Eigen::Vector3d& v, return_value_policy, handle) {
    py::array_t<double> a(3);
    for (int k = 0; k < 3; ++k) a.mutable_data()[k] = v[k];
    return a.release();
  }
};
template <> struct type_caster<Eigen::Matrix3d> {
  PYBIND11_TYPE_CASTER(Eigen::Matrix3d, _("numpy.ndarray[float64[3,3]]"));
  bool load(handle src, bool) {
    auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(src);
    if (!a || a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 3) return false;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) value(r, c) = a.at(r, c);
    return true;
  }
  static handle cast(const Eigen::Matrix3d& m, return_value_policy, handle) {
    py::array_t<double> a({3, 3});
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) a.mutable_at(r, c) = m(r, c);
    return a.release();
  }
};
}}  // namespace pybind11::detail

typedef std::unordered_map<uint32_t, Eigen::Vector3d> OrientationMap;
typedef std::unordered_map<ViewIdPair, TwoViewInfo> EdgeMap;
PYBIND11_MAKE_OPAQUE(OrientationMap);
PYBIND11_MAKE_OPAQUE(EdgeMap);
PYBIND11_MAKE_OPAQUE(CovarianceMap);
PYBIND11_MAKE_OPAQUE(std::vector<double>);

namespace {

// ceres::LossFunction trampoline (bind :33-65) that can also describe itself to the device through an
// optional Python method native_program() -> list of (kind, p0, p1, p2) (globalsfmpy_amd/loss_functions.py).
class PyLoss : public ceres::LossFunction, public gsfm::DescribedLoss {
 public:
  void Evaluate(double sq_norm, double out[3]) const override {
    py::gil_scoped_acquire gil;
    py::function f = py::get_override(static_cast<const ceres::LossFunction*>(this), "Evaluate");
    if (!f) py::pybind11_fail("Tried to call pure virtual function \"LossFunction::Evaluate\"");
    py::array_t<double> buf(3);
    buf.mutable_data()[0] = buf.mutable_data()[1] = buf.mutable_data()[2] = 0.0;
    f(sq_norm, buf);
    for (int k = 0; k < 3; ++k) out[k] = buf.data()[k];
  }
  int NativeProgram(gsfm_loss_node* out, int cap) const override {
    py::gil_scoped_acquire gil;
    py::function f = py::get_override(static_cast<const ceres::LossFunction*>(this), "native_program");
    if (!f) return -1;
    py::object r = f();
    if (r.is_none()) return -1;
    py::list nodes = r.cast<py::list>();
    if ((int)nodes.size() > cap) return -1;
    int n = 0;
    for (auto h : nodes) {
      py::tuple t = h.cast<py::tuple>();
      gsfm_loss_node nd{};
      nd.kind = t[0].cast<int>();
      for (size_t c = 1; c < t.size() && c < 4; ++c) nd.p[c - 1] = t[c].cast<double>();
      out[n++] = nd;
    }
    return n;
  }
};

class PyRotationEstimator : public RotationEstimator {
 public:
  bool EstimateRotations(const EdgeMap& view_pairs, OrientationMap* rotations) override {
    py::gil_scoped_acquire gil;
    PYBIND11_OVERRIDE_PURE(bool, RotationEstimator, EstimateRotations, view_pairs, rotations);
  }
};

// Theia's GlobalRotationEstimatorType (reconstruction_estimator_options.h), names and values
enum class GlobalRotationEstimatorType { ROBUST_L1L2 = 0, NONLINEAR = 1, LINEAR = 2 };
bool ParseGlobalRotationEstimatorType(const std::string& text, GlobalRotationEstimatorType* out) {
  if (text == "ROBUST_L1L2") *out = GlobalRotationEstimatorType::ROBUST_L1L2;
  else if (text == "NONLINEAR") *out = GlobalRotationEstimatorType::NONLINEAR;
  else if (text == "LINEAR") *out = GlobalRotationEstimatorType::LINEAR;
  else return false;
  return true;
}

// --- light stand-ins for the pipeline objects sfm_pipeline.py passes around ---
struct ReconstructionEstimatorOptions {
  // :87 sets ROBUST_L1L2; the default here is NONLINEAR, what both of the reference's flag files choose (a departure: INTEGRATION.md).
  // Read by EstimateGlobalRotationsFromOptions() only; the YAML's global_rotation_estimator.
  GlobalRotationEstimatorType global_rotation_estimator_type = GlobalRotationEstimatorType::NONLINEAR;
  int num_threads = 1;                                       // reconstruction_estimator_options.h:99
  int min_num_two_view_inliers = 30;                         // :107
  double rotation_filtering_max_difference_degrees = 5.0;    // :122
  bool refine_relative_translations_after_rotation_estimation = true;   // :129
  bool filter_relative_translations_with_1dsfm = true;       // :143
  int translation_filtering_num_iterations = 48;             // :146
  double translation_filtering_projection_tolerance = 0.1;   // :149
  double min_triangulation_angle_degrees = 4.0;              // :278
  double triangulation_max_reprojection_error_in_pixels = 15.0;   // :281
  bool bundle_adjust_tracks = true;                          // :284; honoured by EstimateStructure(refine=True) only: the default call does not refine tracks
  std::string bundle_adjustment_loss_function_type = "TRIVIAL";   // :248 (LossFunctionType::TRIVIAL); the YAML's bundle_adjustment_robust_loss_function
  double bundle_adjustment_robust_loss_width = 10.0;         // :251
  int min_cameras_for_iterative_solver = 1000;               // :258; from this many views on BundleAdjustCameraPositionsAndPoints takes 1.5 x the iterations
  double max_reprojection_error_in_pixels = 5.0;             // :115; the outlier rule after a bundle adjustment (the YAML's max_reprojection_error_pixels)
  int num_retriangulation_iterations = 1;                    // :237; the pipeline's structure loop runs 1 + this many times
  bool refine_camera_positions_and_points_after_position_estimation = true;   // :229; the partial adjustment of the loop's first pass
  // :242; which intrinsics BundleAdjustment() moves (the YAML's intrinsics_to_optimize; the reference's flags.yaml sets FOCAL_LENGTH, its
  // flags_1dsfm.yaml NONE).  NONE and FOCAL_LENGTH run on the device; any other bit makes BundleAdjustment() fail with a message.
  gsfm::OptimizeIntrinsicsType intrinsics_to_optimize = gsfm::OptimizeIntrinsicsType::NONE;
  // :282-300; both bundle adjustments hand the solver the tracks of Theia's SelectGoodTracksForBundleAdjustment only (gsfm_tracks_select_good);
  // Theia's header defaults (the reference's flag files say 100 tracks per view)
  bool subsample_tracks_for_bundle_adjustment = false;
  int track_subset_selection_long_track_length_threshold = 10;
  int track_selection_image_grid_cell_size_pixels = 100;
  int min_num_optimized_tracks_per_view = 200;
  // reconstruction_estimator_options.h: what the position stage's estimator is built with (the YAML's position_estimation_min_num_tracks_per_view
  // and position_estimation_robust_loss_width; GlobalReconstructionEstimator.PositionEstimator() hands them over with the reconstruction)
  GSfMNonlinearPositionEstimator::Options nonlinear_position_estimator_options;
};
struct ReconstructionBuilderOptions {
  int num_threads = 1;
  int min_track_length = 2;      // reconstruction_builder.h: what CheckView()'s track builder drops (fewer features) ...
  int max_track_length = 1000;   // ... and where it refuses a union (the YAML's min_track_length / max_track_length)
  ReconstructionEstimatorOptions reconstruction_estimator_options;
};
struct FeaturesAndMatchesDatabase {  // bind :166-170 wraps a RocksDB store; only its path matters to the rotation stage
  std::string path;
};
struct ReconstructionBuilder {
  ReconstructionBuilderOptions options;
  Reconstruction* reconstruction;
  ViewGraph* view_graph;
  // the (options, database) form owns what the COLMAP ingestion fills
  std::shared_ptr<Reconstruction> owned_reconstruction;
  std::shared_ptr<ViewGraph> owned_view_graph;
};

// The flattened inputs of gsfm_cov_estimate as numpy arrays, for inspection and for globalsfmpy_amd.covariance.
py::dict edge_matches_dict(const gsfm::EdgeMatches& em) {
  const py::ssize_t E = (py::ssize_t)em.edges.size();
  py::array_t<uint32_t> edges({E, (py::ssize_t)2});
  for (py::ssize_t e = 0; e < E; ++e) { edges.mutable_at(e, 0) = em.edges[e].first; edges.mutable_at(e, 1) = em.edges[e].second; }
  auto vec = [](const std::vector<double>& v, py::ssize_t cols) {
    py::array_t<double> a({(py::ssize_t)(v.size() / cols), cols});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(double));
    return a;
  };
  py::array_t<uint64_t> ptr((py::ssize_t)em.match_ptr.size());
  std::memcpy(ptr.mutable_data(), em.match_ptr.data(), em.match_ptr.size() * sizeof(uint64_t));
  py::dict d;
  d["edges"] = edges; d["match_ptr"] = ptr; d["matches"] = vec(em.matches, 4); d["intrinsics"] = vec(em.intrinsics, 6);
  d["rot"] = vec(em.rotation, 3); d["trans"] = vec(em.position, 3);
  return d;
}

py::dict l1l2_summary_dict(const gsfm_rot_l1l2_summary& s) {
  py::dict d;
  const int n = std::min<int>(s.num_l1_iterations, GSFM_ROT_L1L2_MAX_L1);
  d["num_l1_iterations"] = s.num_l1_iterations;
  d["num_admm_iterations"] = std::vector<int>(s.num_admm_iterations, s.num_admm_iterations + n);
  d["l1_step"] = std::vector<double>(s.l1_step, s.l1_step + n);
  d["num_irls_iterations"] = s.num_irls_iterations; d["last_irls_step"] = s.last_irls_step;
  d["l1_converged"] = s.l1_converged; d["irls_converged"] = s.irls_converged;
  d["num_cg_iterations"] = s.num_cg_iterations; d["num_linear_solves"] = s.num_linear_solves; d["num_pcg_stalled_solves"] = s.num_pcg_stalled_solves;
  d["worst_accepted_cg_residual"] = s.worst_accepted_cg_residual; d["nonfinite"] = s.nonfinite; d["num_edges_used"] = s.num_edges_used;
  d["t_total_ms"] = s.t_total_ms; d["kernel_ms"] = s.kernel_ms;
  return d;
}

py::dict summary_dict(const gsfm_rot_summary& s) {
  py::dict d;
  d["termination"] = s.termination; d["num_iterations"] = s.num_iterations;
  d["num_successful_steps"] = s.num_successful_steps; d["num_unsuccessful_steps"] = s.num_unsuccessful_steps;
  d["num_residual_sweeps"] = s.num_residual_sweeps; d["num_cg_iterations"] = s.num_cg_iterations;
  d["iters_to_1e6"] = s.iters_to_1e6; d["outer_iterations"] = s.outer_iterations;
  d["initial_cost"] = s.initial_cost; d["final_cost"] = s.final_cost; d["t_total_ms"] = s.t_total_ms;
  d["num_edges_used"] = s.num_edges_used; d["last_weight_change"] = s.last_weight_change;
  d["num_dense_solves"] = s.num_dense_solves; d["num_linearizations"] = s.num_linearizations;
  d["t_linearize_ms"] = s.t_linearize_ms; d["t_sweep_ms"] = s.t_sweep_ms; d["t_cg_ms"] = s.t_cg_ms;
  d["num_inexact_steps"] = s.num_inexact_steps; d["num_forcing_refinements"] = s.num_forcing_refinements; d["num_forcing_restarts"] = s.num_forcing_restarts;
  d["num_pcg_capped_steps"] = s.num_pcg_capped_steps; d["worst_accepted_cg_residual"] = s.worst_accepted_cg_residual;
  return d;
}

// src/GSfM_global_reconstruction_estimator.cpp, the rotation stage only.
class GlobalReconstructionEstimator {
 public:
  explicit GlobalReconstructionEstimator(const ReconstructionEstimatorOptions& o) : options_(o) {}
  // Estimate_BeforeStep3 (:272-293 -> :369-395): min-inlier filter, largest connected component.
  // Camera calibration from priors is out of scope (no cameras here).
  bool FilterInitialViewGraphAndCalibrateCameras(ViewGraph* vg, Reconstruction* rec) {
    view_graph_ = vg; reconstruction_ = rec;
    bool any_counts = false;
    for (const auto& e : vg->GetAllEdges()) any_counts |= e.second.num_verified_matches > 0;
    if (any_counts) {  // match counts need tracks.txt; without them every edge would be dropped
      std::vector<ViewIdPair> drop;
      for (const auto& e : vg->GetAllEdges()) if (e.second.num_verified_matches < options_.min_num_two_view_inliers) drop.push_back(e.first);
      for (const auto& k : drop) vg->RemoveEdge(k.first, k.second);
    }
    RemoveDisconnectedViewPairs(vg);
    return vg->NumEdges() > 0;
  }
  bool InitOrientations() { return OrientationsFromMaximumSpanningTree(*view_graph_, &orientations_); }
  bool EstimateGlobalRotationsNonLinear(ceres::LossFunction* loss, RotationErrorType type) {  // :440-461
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    InitOrientations();
    GSfMNonlinearRotationEstimator est;
    const bool ok = est.EstimateRotationsWithCustomizedLoss(view_graph_->GetAllEdges(), &orientations_, loss, options_.num_threads, type);
    summary_ = est.LastSummary(); error_ = est.LastError();
    return ok;
  }
  bool EstimateGlobalRotationsUncertainty(ceres::LossFunction* loss, CovarianceMap& cov, RotationErrorType type) {  // :463-485
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    InitOrientations();
    GSfMNonlinearRotationEstimator est;
    const bool ok = est.EstimateRotationsWithCustomizedLossAndCovariance(view_graph_->GetAllEdges(), &orientations_, loss,
                                                                          options_.num_threads, cov, type, nullptr);
    summary_ = est.LastSummary(); error_ = est.LastError();
    return ok;
  }
  bool EstimateGlobalRotationsSigmaConsensus(ceres::LossFunction* loss, int iters, double sigma_max) {  // :487-507
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    InitOrientations();
    GSfMNonlinearRotationEstimator est;
    const bool ok = est.EstimateRotationsWithSigmaConsensus(view_graph_->GetAllEdges(), &orientations_, loss, options_.num_threads, iters, sigma_max);
    summary_ = est.LastSummary(); error_ = est.LastError();
    return ok;
  }
  // The reference's argument-less EstimateGlobalRotations() (:397-438): the estimator options_.global_rotation_estimator_type names, from the
  // spanning-tree start.  (The binding EstimateGlobalRotations(loss_func, rotation_error_type) keeps its name and meaning.)
  bool EstimateGlobalRotationsFromOptions() {
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    error_.clear();
    std::memset(&summary_, 0, sizeof(summary_));
    std::memset(&l1l2_summary_, 0, sizeof(l1l2_summary_));
    switch (options_.global_rotation_estimator_type) {
      case GlobalRotationEstimatorType::ROBUST_L1L2: {
        InitOrientations();
        RobustRotationEstimator est{RobustRotationEstimator::Options()};
        const bool ok = est.EstimateRotations(view_graph_->GetAllEdges(), &orientations_);
        l1l2_summary_ = est.LastSummary(); error_ = est.LastError();
        return ok;
      }
      case GlobalRotationEstimatorType::NONLINEAR: {
        InitOrientations();
        GSfMNonlinearRotationEstimator est;
        const bool ok = est.EstimateRotations(view_graph_->GetAllEdges(), &orientations_);
        summary_ = est.LastSummary(); error_ = est.LastError();
        return ok;
      }
      case GlobalRotationEstimatorType::LINEAR:
        error_ = "global_rotation_estimator_type LINEAR: the linear rotation estimator is not built in this library (ROBUST_L1L2 and NONLINEAR are)";
        return false;
    }
    error_ = "global_rotation_estimator_type: no such estimator";
    return false;
  }
  void FilterRotations() {  // :509-524
    FilterViewPairsFromOrientation(orientations_, options_.rotation_filtering_max_difference_degrees, view_graph_);
    for (ViewId v : RemoveDisconnectedViewPairs(view_graph_)) orientations_.erase(v);
  }
  // :526-535: every view pair's position_2 refined with the estimated orientations, from the pair's matched features
  RefineRelativeTranslationsStats OptimizePairwiseTranslations() {
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    if (!options_.refine_relative_translations_after_rotation_estimation || !reconstruction_ || !reconstruction_->matches) return {};
    return RefineRelativeTranslationsWithKnownRotations(*reconstruction_->matches, orientations_, options_.num_threads, view_graph_);
  }
  void FilterRelativeTranslation() {  // :537-563 (extract_maximal_rigid_subgraph, off by default, is not built)
    if (!view_graph_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    if (options_.filter_relative_translations_with_1dsfm) {
      FilterViewPairsFromRelativeTranslationOptions o;
      o.num_threads = options_.num_threads;
      o.num_iterations = options_.translation_filtering_num_iterations;
      o.translation_projection_tolerance = options_.translation_filtering_projection_tolerance;
      o.seed = 1;   // translation_filter_options_.rng->Seed(1) (:551)
      FilterViewPairsFromRelativeTranslation(o, orientations_, view_graph_);
    }
    for (ViewId v : RemoveDisconnectedViewPairs(view_graph_)) orientations_.erase(v);
  }
  // :621-636 with bundle_adjustment = false whatever options_.bundle_adjust_tracks says: every track triangulated by the midpoint method and
  // gated on angle and reprojection error, over the views SetReconstructionFromEstimatedPoses marked, in one device call
  // refine = true honours options_.bundle_adjust_tracks: Theia's BundleAdjustTrack between the midpoint and the gate, in the same device call,
  // with the loss of bundle_adjustment_loss_function_type / bundle_adjustment_robust_loss_width
  // only_unestimated = true is Theia's TrackEstimator::EstimateTracks: the tracks that are estimated already keep their (bundle-adjusted)
  // points, the others are triangulated; the summary then counts those others alone
  gsfm::EstimateStructureStats EstimateStructure(bool refine = false, bool only_unestimated = false) {
    if (!reconstruction_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    gsfm::TrackRefinement r;
    r.loss_function = options_.bundle_adjustment_loss_function_type;
    r.loss_width = options_.bundle_adjustment_robust_loss_width;
    const bool refined = refine && options_.bundle_adjust_tracks;
    structure_ = gsfm::EstimateStructure(options_.min_triangulation_angle_degrees, options_.triangulation_max_reprojection_error_in_pixels, reconstruction_,
                                         refined ? &r : nullptr, only_unestimated);
    structure_refine_asked_ = refine;
    return structure_;
  }
  // reference :565-603 up to the solve: the position estimator over this estimator's options and reconstruction (the reference's
  // EstimatePosition builds it the same way and then calls EstimatePositions on the view graph's edges and the estimated orientations)
  GSfMNonlinearPositionEstimator* PositionEstimator() {
    if (!reconstruction_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    return new GSfMNonlinearPositionEstimator(options_.nonlinear_position_estimator_options, *reconstruction_);
  }
  // Theia's BundleAdjustCameraPositionsAndPoints: positions and points move, orientations and intrinsics are held; the loss of
  // bundle_adjustment_loss_function_type / _width; 100 iterations, x 1.5 from min_cameras_for_iterative_solver views on (Theia's
  // SetBundleAdjustmentOptions).  Returns the reference's bool: the solution is usable.
  bool BundleAdjustCameraPositionsAndPoints() {
    if (!reconstruction_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    int iterations = 100;
    if (reconstruction_->NumViews() >= options_.min_cameras_for_iterative_solver) iterations = (int)(iterations * 1.5);
    // Theia :690-704: with subsample_tracks_for_bundle_adjustment the adjuster is given the selected tracks only; no flag changes and the
    // points outside the subset keep their bytes
    std::vector<uint8_t> subset;
    const bool subsample = SelectTracks(&subset);
    bundle_ = gsfm::BundleAdjustCameraPositionsAndPoints(options_.bundle_adjustment_loss_function_type, options_.bundle_adjustment_robust_loss_width,
                                                         iterations, reconstruction_, subsample ? &subset : nullptr);
    return bundle_.usable;
  }
  // subsample_tracks_for_bundle_adjustment set: the selection over the reconstruction as it stands, true; unset: nothing runs, false
  bool SelectTracks(std::vector<uint8_t>* subset) {
    selection_ = gsfm::TrackSelectionStats();
    if (!options_.subsample_tracks_for_bundle_adjustment) return false;
    selection_ = gsfm::SelectGoodTracksForBundleAdjustment(*reconstruction_, options_.track_subset_selection_long_track_length_threshold,
                                                           options_.track_selection_image_grid_cell_size_pixels, options_.min_num_optimized_tracks_per_view,
                                                           subset);
    return selection_.ran;
  }
  gsfm::TrackSelectionStats selection_;   // of the last bundle adjustment, either kind (ran = false when the option is unset)
  // bind_src/GlobalSfMpy.cpp:591-608: BundleAdjustment(); an unusable solution returns at once and removes nothing; otherwise Theia's
  // SetOutlierTracksToUnestimated with max_reprojection_error_in_pixels and min_triangulation_angle_degrees (gsfm_tracks_outlier_tracks).
  bool BundleAdjustmentAndRemoveOutlierPoints() {
    outlier_ = gsfm::OutlierTracksStats();
    if (!BundleAdjustment()) return false;
    outlier_ = gsfm::SetOutlierTracksToUnestimated(options_.max_reprojection_error_in_pixels, options_.min_triangulation_angle_degrees, reconstruction_);
    return true;
  }
  gsfm::OutlierTracksStats outlier_;     // of the last BundleAdjustmentAndRemoveOutlierPoints (zeros when the adjustment was not usable)
  // Theia's BundleAdjustment (the solve of BundleAdjustmentAndRemoveOutlierPoints; SetOutlierTracksToUnestimated is not part of it): all
  // estimated views and tracks, orientations, positions and points move; loss and iteration rule as above.  The intrinsics follow
  // options.intrinsics_to_optimize: NONE holds them, FOCAL_LENGTH moves every estimated view's focal length too (include/gsfm_ba7.h) and
  // writes it to the reconstruction, where the later calls (the outlier rule, EstimateStructure, the next adjustment) read it; with any
  // other bit nothing runs, the reconstruction is untouched and the call returns false with LastError() naming the unsupported bits.  The
  // new orientations and positions are written back to the reconstruction.
  bool BundleAdjustment() {
    if (!reconstruction_) throw std::runtime_error("call FilterInitialViewGraphAndCalibrateCameras first");
    int iterations = 100;
    if (reconstruction_->NumViews() >= options_.min_cameras_for_iterative_solver) iterations = (int)(iterations * 1.5);
    error_.clear();
    try {
      // Theia :649-663: with subsample_tracks_for_bundle_adjustment every estimated track that was not chosen becomes unestimated first
      // (SetTracksInViewsToUnestimated: it stays so, the outlier rule and the retriangulation see it), then what is left is adjusted.
      // The intrinsics are looked at first, so that an unsupported bit still leaves the reconstruction untouched.
      std::vector<uint8_t> subset;
      if (((int)options_.intrinsics_to_optimize & ~(int)gsfm::OptimizeIntrinsicsType::FOCAL_LENGTH) == 0 && SelectTracks(&subset))
        for (size_t t = 0; t < reconstruction_->track_estimated.size(); ++t)
          if (t >= subset.size() || !subset[t]) reconstruction_->track_estimated[t] = 0;
      bundle_ = gsfm::BundleAdjustment(options_.bundle_adjustment_loss_function_type, options_.bundle_adjustment_robust_loss_width, iterations,
                                       (int)options_.intrinsics_to_optimize, reconstruction_);
    } catch (const std::invalid_argument& e) {
      bundle_ = gsfm::BundleAdjustmentStats();
      bundle_.usable = false;
      error_ = e.what();
      return false;
    }
    return bundle_.usable;
  }
  gsfm::BundleAdjustmentStats bundle_;   // of the last bundle adjustment, either kind
  bool structure_refine_asked_ = false;
  gsfm::EstimateStructureStats structure_;
  ReconstructionEstimatorOptions options_;
  ViewGraph* view_graph_ = nullptr;
  Reconstruction* reconstruction_ = nullptr;
  OrientationMap orientations_;
  gsfm_rot_summary summary_{};
  gsfm_rot_l1l2_summary l1l2_summary_{};   // of EstimateGlobalRotationsFromOptions() under ROBUST_L1L2
  std::string error_;
};

py::dict refine_stats_dict(const RefineRelativeTranslationsStats& st) {
  py::dict d;
  d["num_refined"] = st.num_refined; d["num_skipped"] = st.num_skipped; d["num_nonfinite"] = st.num_nonfinite; d["kernel_ms"] = st.kernel_ms;
  return d;
}

py::dict structure_dict(const gsfm::EstimateStructureStats& st, bool bundle_adjust_tracks, bool refine_asked = false) {
  py::dict d;
  d["num_tracks"] = st.num_tracks; d["num_estimated"] = st.num_estimated; d["kernel_ms"] = st.kernel_ms;
  d["counts"] = std::vector<uint64_t>(st.counts, st.counts + 6);
  d["num_bad_angles"] = st.counts[1] + st.counts[2];                    // what Theia's log calls them
  d["num_failed_triangulations"] = st.counts[3];
  d["num_bad_reprojections"] = st.counts[4] + st.counts[5];
  d["tracks_refined"] = false;
  d["bundle_adjust_tracks_requested"] = bundle_adjust_tracks;
  d["note"] = "tracks triangulated without per-track refinement (bundle_adjust_tracks is not honoured)";
  if (refine_asked) {   // EstimateStructure(refine=True): the option decides
    d["tracks_refined"] = st.tracks_refined;
    d["num_refinement_failed"] = st.num_refinement_failed;
    d["mean_iterations"] = st.mean_iterations;
    d["max_iterations"] = st.max_iterations;
    d["note"] = st.tracks_refined ? "tracks triangulated and refined per track (bundle_adjust_tracks)"
                                  : "tracks triangulated without per-track refinement (bundle_adjust_tracks is false)";
  }
  return d;
}

py::dict bundle_dict(const gsfm::BundleAdjustmentStats& st) {
  py::dict d;
  d["ran"] = st.ran; d["usable"] = st.usable; d["termination"] = st.termination; d["num_iterations"] = st.num_iterations;
  d["num_successful_steps"] = st.num_successful_steps; d["num_unsuccessful_steps"] = st.num_unsuccessful_steps;
  d["num_cg_iterations"] = st.num_cg_iterations; d["max_num_iterations"] = st.max_num_iterations;
  d["num_observations"] = st.num_observations; d["num_cameras"] = st.num_cameras; d["num_points"] = st.num_points;
  d["initial_cost"] = st.initial_cost; d["final_cost"] = st.final_cost; d["t_total_ms"] = st.t_total_ms;
  d["focal_lengths_free"] = st.focal_lengths_free;
  return d;
}

py::dict selection_dict(const gsfm::TrackSelectionStats& st) {
  static const char* const names[6] = {"tracks_with_items", "cells", "selected_by_cell", "cameras_topped_up", "selected_by_top_up", "selected"};
  py::dict d;
  d["ran"] = st.ran;
  for (int k = 0; k < 6; ++k) d[names[k]] = st.counts[k];
  d["long_track_length_threshold"] = st.long_track_length_threshold; d["image_grid_cell_size_pixels"] = st.image_grid_cell_size_pixels;
  d["min_num_optimized_tracks_per_view"] = st.min_num_optimized_tracks_per_view;
  d["num_deficient_items"] = st.num_deficient_items; d["kernel_ms"] = st.kernel_ms; d["replay_ms"] = st.replay_ms;
  return d;
}

py::dict outlier_dict(const gsfm::OutlierTracksStats& st) {
  py::dict d;
  d["num_examined"] = st.num_examined; d["num_removed"] = st.num_removed; d["kernel_ms"] = st.kernel_ms;
  d["counts"] = std::vector<uint64_t>(st.counts, st.counts + 5);
  d["num_bad_reprojections"] = st.counts[2] + st.counts[3];            // what Theia's log calls them
  d["num_insufficient_viewing_angles"] = st.counts[4];
  return d;
}

py::dict pos_summary_dict(const gsfm_pos_summary& s) {
  py::dict d;
  d["termination"] = s.termination; d["num_iterations"] = s.num_iterations;
  d["num_successful_steps"] = s.num_successful_steps; d["num_unsuccessful_steps"] = s.num_unsuccessful_steps;
  d["num_cg_iterations"] = s.num_cg_iterations; d["num_dense_solves"] = s.num_dense_solves; d["num_pcg_stalled_steps"] = s.num_pcg_stalled_steps;
  d["num_residual_sweeps"] = s.num_residual_sweeps; d["num_linearizations"] = s.num_linearizations; d["nonfinite"] = s.nonfinite;
  d["num_edges_used"] = s.num_edges_used; d["initial_cost"] = s.initial_cost; d["final_cost"] = s.final_cost;
  d["final_gradient_max_norm"] = s.final_gradient_max_norm; d["final_radius"] = s.final_radius; d["max_radius"] = s.max_radius;
  d["t_total_ms"] = s.t_total_ms;
  return d;
}

void load_1dsfm_config(const std::string& flagfile, ReconstructionBuilderOptions& options) {
  // bind :185-271 parses the YAML with yaml-cpp; only the keys the rotation stage consumes are read here.
  py::gil_scoped_acquire gil;
  py::object cfg = py::module_::import("yaml").attr("safe_load")(py::module_::import("builtins").attr("open")(flagfile));
  auto get = [&](const char* k, auto& dst) { if (cfg.contains(k) && !cfg[k].is_none()) dst = cfg[k].cast<std::decay_t<decltype(dst)>>(); };
  get("num_threads", options.num_threads);
  options.reconstruction_estimator_options.num_threads = options.num_threads;
  get("min_track_length", options.min_track_length);   // bind :189-190
  get("max_track_length", options.max_track_length);
  get("min_num_inliers_for_valid_match", options.reconstruction_estimator_options.min_num_two_view_inliers);
  get("post_rotation_filtering_degrees", options.reconstruction_estimator_options.rotation_filtering_max_difference_degrees);
  get("refine_relative_translations_after_rotation_estimation", options.reconstruction_estimator_options.refine_relative_translations_after_rotation_estimation);
  get("filter_relative_translations_with_1dsfm", options.reconstruction_estimator_options.filter_relative_translations_with_1dsfm);
  get("min_triangulation_angle_degrees", options.reconstruction_estimator_options.min_triangulation_angle_degrees);
  get("triangulation_reprojection_error_pixels", options.reconstruction_estimator_options.triangulation_max_reprojection_error_in_pixels);
  get("bundle_adjust_tracks", options.reconstruction_estimator_options.bundle_adjust_tracks);
  get("bundle_adjustment_robust_loss_function", options.reconstruction_estimator_options.bundle_adjustment_loss_function_type);
  get("bundle_adjustment_robust_loss_width", options.reconstruction_estimator_options.bundle_adjustment_robust_loss_width);
  get("min_cameras_for_iterative_solver", options.reconstruction_estimator_options.min_cameras_for_iterative_solver);
  get("max_reprojection_error_pixels", options.reconstruction_estimator_options.max_reprojection_error_in_pixels);
  get("num_retriangulation_iterations", options.reconstruction_estimator_options.num_retriangulation_iterations);
  get("refine_camera_positions_and_points_after_position_estimation",
      options.reconstruction_estimator_options.refine_camera_positions_and_points_after_position_estimation);
  get("subsample_tracks_for_bundle_adjustment", options.reconstruction_estimator_options.subsample_tracks_for_bundle_adjustment);   // bind :261-270
  get("track_subset_selection_long_track_length_threshold", options.reconstruction_estimator_options.track_subset_selection_long_track_length_threshold);
  get("track_selection_image_grid_cell_size_pixels", options.reconstruction_estimator_options.track_selection_image_grid_cell_size_pixels);
  get("min_num_optimized_tracks_per_view", options.reconstruction_estimator_options.min_num_optimized_tracks_per_view);
  get("position_estimation_min_num_tracks_per_view", options.reconstruction_estimator_options.nonlinear_position_estimator_options.min_num_points_per_view);   // bind :228-230
  get("position_estimation_robust_loss_width", options.reconstruction_estimator_options.nonlinear_position_estimator_options.robust_loss_width);
  std::string rotation_estimator;   // bind :213-214 (StringToRotationEstimatorType); an absent key leaves this library's default, NONLINEAR
  get("global_rotation_estimator", rotation_estimator);
  if (!rotation_estimator.empty() && !ParseGlobalRotationEstimatorType(rotation_estimator, &options.reconstruction_estimator_options.global_rotation_estimator_type))
    throw std::invalid_argument(flagfile + ": global_rotation_estimator: no such estimator '" + rotation_estimator + "' (ROBUST_L1L2, NONLINEAR, LINEAR)");
  // bind :199-200: a bitmask of names joined by '|' (StringToOptimizeIntrinsicsType); an absent key leaves NONE
  std::string intrinsics;
  get("intrinsics_to_optimize", intrinsics);
  if (cfg.contains("intrinsics_to_optimize") && !cfg["intrinsics_to_optimize"].is_none()) {
    int mask = 0;
    std::string error;
    if (!gsfm::ParseOptimizeIntrinsicsType(intrinsics, &mask, &error)) throw std::invalid_argument(flagfile + ": " + error);
    options.reconstruction_estimator_options.intrinsics_to_optimize = (gsfm::OptimizeIntrinsicsType)mask;
  }
}

}  // namespace

PYBIND11_MODULE(_GlobalSfMpy, m) {  // imported through the GlobalSfMpy.py shim beside it (HIP runtime pre-load)
  m.doc() = "MI355X-native drop-in for the rotation-averaging surface of zhangganlin/GlobalSfMpy";

  py::bind_map<OrientationMap>(m, "MapViewIdVector3d");
  py::bind_map<EdgeMap>(m, "MapEdges");
  py::bind_map<CovarianceMap>(m, "MapEdgesCovariance");
  py::bind_vector<std::vector<double>>(m, "VectorDouble");

  py::enum_<RotationErrorType>(m, "RotationErrorType", py::arithmetic())  // the 7 values the reference binds (:431-439)
      .value("QUATERNION_COSINE", RotationErrorType::QUATERNION_COSINE)
      .value("QUATERNION_NORM", RotationErrorType::QUATERNION_NORM)
      .value("ROTATION_MAT_FNORM", RotationErrorType::ROTATION_MAT_FNORM)
      .value("ANGLE_AXIS_COVARIANCE", RotationErrorType::ANGLE_AXIS_COVARIANCE)
      .value("ANGLE_AXIS", RotationErrorType::ANGLE_AXIS)
      .value("ANGLE_AXIS_COVTRACE", RotationErrorType::ANGLE_AXIS_COVTRACE)
      .value("ANGLE_AXIS_COVNORM", RotationErrorType::ANGLE_AXIS_COVNORM);
  py::enum_<PositionErrorType>(m, "PositionErrorType", py::arithmetic()).value("BASELINE", PositionErrorType::BASELINE);   // the one value bound

  py::class_<ceres::LossFunction, PyLoss>(m, "LossFunction").def(py::init<>());

  py::class_<RotationEstimator, PyRotationEstimator>(m, "RotationEstimator")
      .def(py::init<>())
      .def("EstimateRotations", &RotationEstimator::EstimateRotations);

  // reference src/GSfM_nonlinear_position_estimator.cpp on the device (include/gsfm_pos.h): fills `positions` in place; the view held
  // constant is positions->begin() of the map, as in the reference (FixedView() tells which)
  py::class_<GSfMNonlinearPositionEstimator::Options>(m, "NonlinearPositionEstimatorOptions")
      .def(py::init<>())
      .def_readwrite("num_threads", &GSfMNonlinearPositionEstimator::Options::num_threads)
      .def_readwrite("max_num_iterations", &GSfMNonlinearPositionEstimator::Options::max_num_iterations)
      .def_readwrite("robust_loss_width", &GSfMNonlinearPositionEstimator::Options::robust_loss_width)
      .def_readwrite("min_num_points_per_view", &GSfMNonlinearPositionEstimator::Options::min_num_points_per_view)
      .def_readwrite("point_to_camera_weight", &GSfMNonlinearPositionEstimator::Options::point_to_camera_weight)
      .def_readwrite("rays_from_reconstruction_orientation", &GSfMNonlinearPositionEstimator::Options::rays_from_reconstruction_orientation);
  // include/gsfm/position_track_selection.hpp: the tracks of the point-to-camera constraints and their weight, on a track CSR over view ids
  m.def("SelectTracksForPositionEstimation", [](const std::vector<uint32_t>& positioned_views, const std::vector<uint64_t>& track_ptr,
                                                const std::vector<uint32_t>& obs_view, int min_num_points_per_view) {
    if (track_ptr.empty() || track_ptr[0] != 0 || track_ptr.back() != obs_view.size()) throw std::invalid_argument("track_ptr does not describe obs_view");
    for (size_t t = 0; t + 1 < track_ptr.size(); ++t) if (track_ptr[t + 1] < track_ptr[t]) throw std::invalid_argument("track_ptr decreases");
    const gsfm::PositionTrackSelection sel = gsfm::SelectTracksForPositionEstimation(positioned_views, track_ptr.size() - 1, track_ptr.data(), obs_view.data(),
                                                                                      min_num_points_per_view);
    py::dict d, credits;
    for (const auto& kv : sel.credits) credits[py::int_(kv.first)] = kv.second;
    d["tracks"] = sel.tracks; d["credits"] = credits; d["num_point_to_camera_constraints"] = sel.num_point_to_camera_constraints;
    return d;
  });
  m.def("PointToCameraWeight", &gsfm::PointToCameraWeight);
  py::class_<GSfMNonlinearPositionEstimator>(m, "NonlinearPositionEstimator")
      .def(py::init<>())
      .def(py::init<const GSfMNonlinearPositionEstimator::Options&>())
      .def(py::init<const GSfMNonlinearPositionEstimator::Options&, const Reconstruction&>(), py::keep_alive<1, 3>())   // the reference's constructor
      .def_property_readonly("options", [](GSfMNonlinearPositionEstimator& e) { return e.MutableEstimatorOptions(); }, py::return_value_policy::reference_internal)
      .def("LastPointConstraints", [](const GSfMNonlinearPositionEstimator& e) {
        const GSfMNonlinearPositionEstimator::PointConstraints& p = e.LastPointConstraints();
        py::dict d;
        d["num_tracks"] = p.num_tracks; d["num_constraints"] = p.num_constraints; d["num_observations_used"] = p.num_observations_used;
        d["num_active_points"] = p.num_active_points; d["weight"] = p.weight;
        return d;
      })
      .def(py::init([](int max_num_iterations, double robust_loss_width) {
             GSfMNonlinearPositionEstimator::Options o;
             o.max_num_iterations = max_num_iterations; o.robust_loss_width = robust_loss_width;
             return new GSfMNonlinearPositionEstimator(o);
           }), py::arg("max_num_iterations") = 400, py::arg("robust_loss_width") = 0.1)
      .def("EstimatePositions",
           [](GSfMNonlinearPositionEstimator& e, const EdgeMap& vp, const OrientationMap& o, OrientationMap* positions, ceres::LossFunction* loss,
              PositionErrorType type) { return e.EstimatePositions(vp, o, positions, type, loss); },
           py::arg("view_pairs"), py::arg("orientations"), py::arg("positions"), py::arg("loss_function") = nullptr,
           py::arg("position_error_type") = PositionErrorType::BASELINE, py::call_guard<py::gil_scoped_release>())
      .def("FixedView", &GSfMNonlinearPositionEstimator::FixedView)
      .def("LastSummary", [](const GSfMNonlinearPositionEstimator& e) { return pos_summary_dict(e.LastSummary()); })
      .def("LastError", [](const GSfMNonlinearPositionEstimator& e) { return std::string(e.LastError()); })
      .def("SetSolverOption", [](GSfMNonlinearPositionEstimator& e, const std::string& name, double v) {   // a few fields of gsfm_pos_options
        gsfm_pos_options* o = e.MutableOptions();
        if (name == "dense_max_cams") o->dense_max_cams = (int32_t)v;
        else if (name == "remove_scale_gauge") o->remove_scale_gauge = (int32_t)v;
        else if (name == "cg_relative_tolerance") o->cg_relative_tolerance = v;
        else throw std::invalid_argument("unknown position solver option " + name);
      });

  py::class_<GSfMNonlinearRotationEstimator, RotationEstimator>(m, "NonlinearRotationEstimator")
      .def(py::init<>())
      .def(py::init<const double>())
      .def("EstimateRotations", &GSfMNonlinearRotationEstimator::EstimateRotations, py::call_guard<py::gil_scoped_release>())
      .def("EstimateRotationsWithCustomizedLoss", &GSfMNonlinearRotationEstimator::EstimateRotationsWithCustomizedLoss,
           py::arg("view_pairs"), py::arg("global_orientations"), py::arg("loss_function"), py::arg("thread_num"),
           py::arg("rotation_error_type") = RotationErrorType::QUATERNION_COSINE, py::call_guard<py::gil_scoped_release>())
      .def("EstimateRotationsWithCustomizedLossAndCovariance",
           [](GSfMNonlinearRotationEstimator& e, const EdgeMap& vp, OrientationMap* o, ceres::LossFunction* l, int threads, CovarianceMap& c,
              RotationErrorType t) { py::gil_scoped_release rel; return e.EstimateRotationsWithCustomizedLossAndCovariance(vp, o, l, threads, c, t, nullptr); })
      .def("EstimateRotationsWithSigmaConsensus", &GSfMNonlinearRotationEstimator::EstimateRotationsWithSigmaConsensus,
           py::call_guard<py::gil_scoped_release>())
      .def("LastSummary", [](const GSfMNonlinearRotationEstimator& e) { return summary_dict(e.LastSummary()); })
      .def("LastError", [](const GSfMNonlinearRotationEstimator& e) { return std::string(e.LastError()); });

  py::class_<RobustRotationEstimator::Options>(m, "RobustRotationEstimatorOptions")
      .def(py::init<>())
      .def_readwrite("max_num_l1_iterations", &RobustRotationEstimator::Options::max_num_l1_iterations)
      .def_readwrite("l1_step_convergence_threshold", &RobustRotationEstimator::Options::l1_step_convergence_threshold)
      .def_readwrite("max_num_irls_iterations", &RobustRotationEstimator::Options::max_num_irls_iterations)
      .def_readwrite("irls_step_convergence_threshold", &RobustRotationEstimator::Options::irls_step_convergence_threshold)
      .def_readwrite("irls_loss_parameter_sigma", &RobustRotationEstimator::Options::irls_loss_parameter_sigma);
  py::class_<RobustRotationEstimator, RotationEstimator>(m, "RobustRotationEstimator")
      .def(py::init<>())
      .def(py::init<const RobustRotationEstimator::Options&>())
      .def("EstimateRotations", py::overload_cast<const EdgeMap&, OrientationMap*>(&RobustRotationEstimator::EstimateRotations),
           py::call_guard<py::gil_scoped_release>())
      .def("EstimateRotations", py::overload_cast<OrientationMap*>(&RobustRotationEstimator::EstimateRotations), py::call_guard<py::gil_scoped_release>())
      .def("AddRelativeRotationConstraint", &RobustRotationEstimator::AddRelativeRotationConstraint)
      .def("FixedView", &RobustRotationEstimator::FixedView)
      .def("LastSummary", [](const RobustRotationEstimator& e) { return l1l2_summary_dict(e.LastSummary()); })
      .def("LastError", [](const RobustRotationEstimator& e) { return std::string(e.LastError()); });
  py::enum_<GlobalRotationEstimatorType>(m, "GlobalRotationEstimatorType")   // Theia's names and values
      .value("ROBUST_L1L2", GlobalRotationEstimatorType::ROBUST_L1L2)
      .value("NONLINEAR", GlobalRotationEstimatorType::NONLINEAR)
      .value("LINEAR", GlobalRotationEstimatorType::LINEAR);

  m.def("test_loss_with_input_x", [](ceres::LossFunction* loss, double x) {  // bind :179-183
    double out[3] = {0, 0, 0};
    loss->Evaluate(x, out);
    py::print("[" + std::to_string(out[0]) + ", " + std::to_string(out[1]) + ", " + std::to_string(out[2]) + "]");
  });

  py::enum_<gsfm::OptimizeIntrinsicsType>(m, "OptimizeIntrinsicsType", py::arithmetic())   // Theia's names and values (a bitmask)
      .value("NONE", gsfm::OptimizeIntrinsicsType::NONE)
      .value("FOCAL_LENGTH", gsfm::OptimizeIntrinsicsType::FOCAL_LENGTH)
      .value("ASPECT_RATIO", gsfm::OptimizeIntrinsicsType::ASPECT_RATIO)
      .value("SKEW", gsfm::OptimizeIntrinsicsType::SKEW)
      .value("PRINCIPAL_POINTS", gsfm::OptimizeIntrinsicsType::PRINCIPAL_POINTS)
      .value("RADIAL_DISTORTION", gsfm::OptimizeIntrinsicsType::RADIAL_DISTORTION)
      .value("TANGENTIAL_DISTORTION", gsfm::OptimizeIntrinsicsType::TANGENTIAL_DISTORTION)
      .value("ALL", gsfm::OptimizeIntrinsicsType::ALL);
  m.def("StringToOptimizeIntrinsicsType", [](const std::string& text) {
    int mask = 0;
    std::string error;
    if (!gsfm::ParseOptimizeIntrinsicsType(text, &mask, &error)) throw std::invalid_argument(error);
    return mask;
  });
  m.def("ba7_abi_version", [] { return GSFM_BA7_ABI_VERSION; });   // the header this module was compiled against

  py::class_<ReconstructionEstimatorOptions>(m, "ReconstructionEstimatorOptions")
      .def(py::init<>())
      .def_property("intrinsics_to_optimize", [](const ReconstructionEstimatorOptions& o) { return py::cast(o.intrinsics_to_optimize); },
                    [](ReconstructionEstimatorOptions& o, int mask) {   // an enum value, or an | of them (an int)
                      if (mask & ~(int)gsfm::OptimizeIntrinsicsType::ALL) throw std::invalid_argument("intrinsics_to_optimize: no such bit");
                      o.intrinsics_to_optimize = (gsfm::OptimizeIntrinsicsType)mask;
                    })
      .def_readwrite("global_rotation_estimator_type", &ReconstructionEstimatorOptions::global_rotation_estimator_type)
      .def_readwrite("num_threads", &ReconstructionEstimatorOptions::num_threads)
      .def_readwrite("min_num_two_view_inliers", &ReconstructionEstimatorOptions::min_num_two_view_inliers)
      .def_readwrite("rotation_filtering_max_difference_degrees", &ReconstructionEstimatorOptions::rotation_filtering_max_difference_degrees)
      .def_readwrite("refine_relative_translations_after_rotation_estimation", &ReconstructionEstimatorOptions::refine_relative_translations_after_rotation_estimation)
      .def_readwrite("filter_relative_translations_with_1dsfm", &ReconstructionEstimatorOptions::filter_relative_translations_with_1dsfm)
      .def_readwrite("translation_filtering_num_iterations", &ReconstructionEstimatorOptions::translation_filtering_num_iterations)
      .def_readwrite("translation_filtering_projection_tolerance", &ReconstructionEstimatorOptions::translation_filtering_projection_tolerance)
      .def_readwrite("min_triangulation_angle_degrees", &ReconstructionEstimatorOptions::min_triangulation_angle_degrees)
      .def_readwrite("triangulation_max_reprojection_error_in_pixels", &ReconstructionEstimatorOptions::triangulation_max_reprojection_error_in_pixels)
      .def_readwrite("bundle_adjust_tracks", &ReconstructionEstimatorOptions::bundle_adjust_tracks)
      .def_readwrite("bundle_adjustment_loss_function_type", &ReconstructionEstimatorOptions::bundle_adjustment_loss_function_type)
      .def_readwrite("bundle_adjustment_robust_loss_width", &ReconstructionEstimatorOptions::bundle_adjustment_robust_loss_width)
      .def_readwrite("min_cameras_for_iterative_solver", &ReconstructionEstimatorOptions::min_cameras_for_iterative_solver)
      .def_readwrite("max_reprojection_error_in_pixels", &ReconstructionEstimatorOptions::max_reprojection_error_in_pixels)
      .def_readwrite("num_retriangulation_iterations", &ReconstructionEstimatorOptions::num_retriangulation_iterations)
      .def_readwrite("refine_camera_positions_and_points_after_position_estimation",
                     &ReconstructionEstimatorOptions::refine_camera_positions_and_points_after_position_estimation)
      .def_readwrite("subsample_tracks_for_bundle_adjustment", &ReconstructionEstimatorOptions::subsample_tracks_for_bundle_adjustment)
      .def_readwrite("track_subset_selection_long_track_length_threshold", &ReconstructionEstimatorOptions::track_subset_selection_long_track_length_threshold)
      .def_readwrite("track_selection_image_grid_cell_size_pixels", &ReconstructionEstimatorOptions::track_selection_image_grid_cell_size_pixels)
      .def_readwrite("min_num_optimized_tracks_per_view", &ReconstructionEstimatorOptions::min_num_optimized_tracks_per_view)
      .def_readwrite("nonlinear_position_estimator_options", &ReconstructionEstimatorOptions::nonlinear_position_estimator_options);
  py::class_<ReconstructionBuilderOptions>(m, "ReconstructionBuilderOptions")
      .def(py::init<>())
      .def_readwrite("num_threads", &ReconstructionBuilderOptions::num_threads)
      .def_readwrite("min_track_length", &ReconstructionBuilderOptions::min_track_length)
      .def_readwrite("max_track_length", &ReconstructionBuilderOptions::max_track_length)
      .def_readwrite("reconstruction_estimator_options", &ReconstructionBuilderOptions::reconstruction_estimator_options);
  m.def("load_1DSFM_config", &load_1dsfm_config);

  py::class_<Reconstruction>(m, "Reconstruction")
      .def(py::init<>())
      .def("NumTracks", &Reconstruction::NumTracks)
      .def("NumViews", &Reconstruction::NumViews)
      .def("NumEstimatedTracks", &Reconstruction::NumEstimatedTracks)
      // what CheckView()'s track builder reported (gsfm_tracks_build's counts by name); None when the tracks were not built from matches
      .def("LastTrackBuildSummary", [](const Reconstruction& r) -> py::object {
        if (!r.track_build) return py::none();
        const gsfm::TrackBuildStats& s = *r.track_build;
        static const char* names[7] = {"features", "components", "small", "inconsistent", "degenerate", "replayed", "tracks"};
        py::dict d;
        d["built"] = s.built; d["error"] = s.error;
        for (int k = 0; k < 7; ++k) d[names[k]] = s.counts[k];
        d["num_matches"] = s.num_matches; d["num_tracks"] = s.num_tracks; d["num_observations"] = s.num_observations;
        d["min_track_length"] = s.min_track_length; d["max_track_length"] = s.max_track_length; d["kernel_ms"] = s.kernel_ms;
        return d;
      })
      // the focal length a bundle adjustment with FOCAL_LENGTH estimated for the view, or None (FlattenedTracks() shows what is in use)
      .def("ViewFocalLength", [](const Reconstruction& r, ViewId v) -> py::object {
        const auto it = r.focal_length.find(v);
        return it == r.focal_length.end() ? py::object(py::none()) : py::object(py::float_(it->second));
      })
      .def("SetViewFocalLength", [](Reconstruction& r, ViewId v, double f) {
        if (!(f > 0.0) || !std::isfinite(f)) throw std::invalid_argument("a focal length must be finite and positive");
        r.focal_length[v] = f;
      })
      // a track is addressed by its index in tracks.txt (Theia's TrackId of a 1DSfM dataset); Track(id)->Point(), IsEstimated(), NumViews()
      .def("TrackPoint", [](const Reconstruction& r, size_t t) {
        if (t >= (size_t)r.NumTracks()) throw py::index_error("no such track");
        return t < r.track_point.size() ? r.track_point[t] : Eigen::Vector3d();
      })
      .def("TrackIsEstimated", [](const Reconstruction& r, size_t t) {
        if (t >= (size_t)r.NumTracks()) throw py::index_error("no such track");
        return t < r.track_estimated.size() && r.track_estimated[t] != 0;
      })
      .def("TrackNumViews", [](const Reconstruction& r, size_t t) {
        if (t >= (size_t)r.NumTracks()) throw py::index_error("no such track");
        return (int)r.tracks->tracks[t].size();
      })
      .def("EstimatedTrackIds", [](const Reconstruction& r) {
        std::vector<size_t> ids;
        for (size_t t = 0; t < r.track_estimated.size(); ++t) if (r.track_estimated[t]) ids.push_back(t);
        return ids;
      })
      // the flat arrays EstimateStructure() hands to gsfm_tracks_triangulate (solver.triangulate_tracks takes the same)
      // only_unestimated: the sub-batch EstimateStructure(only_unestimated=True) runs (gsfm::KeepUnestimatedTracks), plus track_index
      .def("FlattenedTracks", [](const Reconstruction& r, bool only_unestimated) -> py::object {
        if (!r.tracks) return py::none();
        gsfm::FlatTracks f;
        gsfm::FlattenTracks(r, &f);
        std::vector<uint64_t> track_index;
        if (only_unestimated) gsfm::KeepUnestimatedTracks(r, &f, &track_index);
        auto arr = [](const auto& v, py::ssize_t cols) {
          using T = typename std::decay_t<decltype(v)>::value_type;
          py::array_t<T> a = cols > 1 ? py::array_t<T>({(py::ssize_t)(v.size() / cols), cols}) : py::array_t<T>((py::ssize_t)v.size());
          if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
          return a;
        };
        py::dict d;
        d["views"] = arr(f.views, 1); d["rot_aa"] = arr(f.rot_aa, 3); d["cam_pos"] = arr(f.cam_pos, 3); d["intrinsics"] = arr(f.intrinsics, 3);
        d["cam_estimated"] = arr(f.cam_estimated, 1); d["track_ptr"] = arr(f.track_ptr, 1); d["obs_cam"] = arr(f.obs_cam, 1); d["obs_xy"] = arr(f.obs_xy, 2);
        if (only_unestimated) d["track_index"] = arr(track_index, 1);
        return d;
      }, py::arg("only_unestimated") = false)
      // what EstimateStructure stores per track, settable (a reconstruction assembled by hand)
      .def("SetTrack", [](Reconstruction& r, size_t t, const Eigen::Vector3d& point, bool estimated) {
        if (t >= (size_t)r.NumTracks()) throw py::index_error("no such track");
        r.track_point.resize((size_t)r.NumTracks(), Eigen::Vector3d(0, 0, 0));
        r.track_estimated.resize((size_t)r.NumTracks(), 0);
        r.track_point[t] = point; r.track_estimated[t] = estimated;
      })
      .def("EstimatedOrientations", [](const Reconstruction& r) { return r.orientation; })
      .def("EstimatedPositions", [](const Reconstruction& r) { return r.position; })
      .def("ViewNames", [](const Reconstruction& r) { return r.view_names; })
      .def("SetViewName", [](Reconstruction& r, ViewId v, const std::string& name) { r.views.insert(v); r.view_names[v] = name; })
      .def("SetOrientation", [](Reconstruction& r, ViewId v, const Eigen::Vector3d& aa) { r.views.insert(v); r.orientation[v] = aa; })
      .def("MatchedFeatures", [](const Reconstruction& r) { return r.matches ? py::object(edge_matches_dict(*r.matches)) : py::object(py::none()); })
      .def("NumMatchedPairs", [](const Reconstruction& r) { return r.matches ? (int)r.matches->edges.size() : 0; });

  py::class_<ViewGraph>(m, "ViewGraph")
      .def(py::init<>())
      .def("NumViews", &ViewGraph::NumViews)
      .def("NumEdges", &ViewGraph::NumEdges)
      .def("HasView", &ViewGraph::HasView)
      .def("HasEdge", &ViewGraph::HasEdge)
      .def("ViewIds", &ViewGraph::ViewIds)
      .def("AddEdge", &ViewGraph::AddEdge)
      .def("RemoveEdge", &ViewGraph::RemoveEdge)
      .def("GetEdge", &ViewGraph::GetEdge, py::return_value_policy::reference_internal)
      .def("GetAllEdges", &ViewGraph::GetAllEdges, py::return_value_policy::reference);

  py::class_<TwoViewInfo>(m, "TwoViewInfo")
      .def(py::init<>())
      .def_readwrite("focal_length_1", &TwoViewInfo::focal_length_1)
      .def_readwrite("focal_length_2", &TwoViewInfo::focal_length_2)
      .def_readwrite("position_2", &TwoViewInfo::position_2)
      .def_readwrite("rotation_2", &TwoViewInfo::rotation_2)
      .def_readwrite("num_verified_matches", &TwoViewInfo::num_verified_matches)
      .def_readwrite("num_homography_inliers", &TwoViewInfo::num_homography_inliers)
      .def_readwrite("visibility_score", &TwoViewInfo::visibility_score);

  py::class_<ReconstructionBuilder>(m, "ReconstructionBuilder")
      .def(py::init([](ReconstructionBuilderOptions& o, Reconstruction* r, ViewGraph* g) { return new ReconstructionBuilder{o, r, g}; }),
           py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def(py::init([](ReconstructionBuilderOptions& o, FeaturesAndMatchesDatabase*) {  // sfm_pipeline.py:46
        auto* b = new ReconstructionBuilder{o, nullptr, nullptr, std::make_shared<Reconstruction>(), std::make_shared<ViewGraph>()};
        b->reconstruction = b->owned_reconstruction.get();
        b->view_graph = b->owned_view_graph.get();
        return b;
      }))
      // views of the graph become views of the reconstruction; a reconstruction that has matches and no tracks gets its tracks built from
      // them (src/GSfM_reconstruction_builder.cpp:441-444 -> Theia's TrackBuilder): the COLMAP branch.  Read1DSFM's tracks are left alone.
      .def("CheckView", [](ReconstructionBuilder& b) {
        Reconstruction* rec = b.reconstruction;
        for (ViewId v : b.view_graph->ViewIds()) rec->views.insert(v);
        if (rec->NumTracks() != 0 || !rec->matches) return;
        auto tracks = std::make_shared<gsfm::Tracks1DSfM>();
        auto stats = std::make_shared<gsfm::TrackBuildStats>();
        try {
          py::gil_scoped_release release;
          *stats = gsfm::BuildTracksFromMatches(*rec->matches, b.options.min_track_length, b.options.max_track_length, tracks.get());
        } catch (const gsfm::NoDeviceError& e) {
          // Without a device nothing after this call runs either.  The reconstruction stays as the ingestion left it -- views and matches, no
          // tracks -- and says so: a warning here, built = false in LastTrackBuildSummary().  Every other failure of the builder is raised.
          stats->built = false; stats->error = e.what();
          stats->min_track_length = b.options.min_track_length; stats->max_track_length = b.options.max_track_length;
          rec->track_build = stats;
          if (PyErr_WarnEx(PyExc_RuntimeWarning, (std::string("CheckView: no tracks were built from the matches: ") + e.what()).c_str(), 1) < 0) throw py::error_already_set();
          return;
        }
        for (const auto& kv : tracks->keypoints) {
          const auto name = rec->view_names.find(kv.first);
          tracks->names[kv.first] = name == rec->view_names.end() ? std::to_string(kv.first) : name->second;
        }
        rec->track_point.clear();
        rec->track_estimated.clear();
        rec->tracks = tracks;
        rec->track_build = stats;
      })
      // reference_internal: the (options, database) form owns both objects, so they must keep the builder alive
      .def("get_view_graph", [](ReconstructionBuilder& b) { return b.view_graph; }, py::return_value_policy::reference_internal)
      .def("get_reconstruction", [](ReconstructionBuilder& b) { return b.reconstruction; }, py::return_value_policy::reference_internal);

  py::class_<GlobalReconstructionEstimator>(m, "GlobalReconstructionEstimator")
      .def(py::init<const ReconstructionEstimatorOptions&>())
      .def("get_view_graph", [](GlobalReconstructionEstimator* e) { return e->view_graph_; }, py::return_value_policy::reference)
      .def("get_reconstruction", [](GlobalReconstructionEstimator* e) { return e->reconstruction_; }, py::return_value_policy::reference)
      .def_readwrite("orientations", &GlobalReconstructionEstimator::orientations_)
      .def_readwrite("options", &GlobalReconstructionEstimator::options_)
      .def("FilterInitialViewGraphAndCalibrateCameras", &GlobalReconstructionEstimator::FilterInitialViewGraphAndCalibrateCameras,
           py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
      .def("OrientationsFromMaximumSpanningTree", &GlobalReconstructionEstimator::InitOrientations)
      .def("EstimateGlobalRotations", &GlobalReconstructionEstimator::EstimateGlobalRotationsNonLinear, py::arg("loss_func") = nullptr,
           py::arg("rotation_error_type") = RotationErrorType::QUATERNION_COSINE, py::call_guard<py::gil_scoped_release>())
      .def("EstimateGlobalRotationsUncertainty", &GlobalReconstructionEstimator::EstimateGlobalRotationsUncertainty,
           py::call_guard<py::gil_scoped_release>())
      .def("EstimateGlobalRotationsWithSigmaConsensus", &GlobalReconstructionEstimator::EstimateGlobalRotationsSigmaConsensus,
           py::call_guard<py::gil_scoped_release>())
      .def("EstimateGlobalRotationsFromOptions", &GlobalReconstructionEstimator::EstimateGlobalRotationsFromOptions, py::call_guard<py::gil_scoped_release>())
      .def("LastRobustRotationSummary", [](const GlobalReconstructionEstimator& e) { return l1l2_summary_dict(e.l1l2_summary_); })
      .def("FilterRotations", &GlobalReconstructionEstimator::FilterRotations)
      .def("OptimizePairwiseTranslations", [](GlobalReconstructionEstimator& e) {
        RefineRelativeTranslationsStats st;
        { py::gil_scoped_release release; st = e.OptimizePairwiseTranslations(); }
        return refine_stats_dict(st);
      })
      .def("FilterRelativeTranslation", &GlobalReconstructionEstimator::FilterRelativeTranslation, py::call_guard<py::gil_scoped_release>())
      // the position stage's estimator with this estimator's nonlinear_position_estimator_options and its reconstruction (the tracks of the
      // point-to-camera constraints); the caller runs EstimatePositions(view_graph edges, orientations, positions, loss)
      .def("PositionEstimator", &GlobalReconstructionEstimator::PositionEstimator, py::return_value_policy::take_ownership, py::keep_alive<0, 1>())
      .def("EstimateStructure", [](GlobalReconstructionEstimator& e, bool refine, bool only_unestimated) {
        gsfm::EstimateStructureStats st;
        { py::gil_scoped_release release; st = e.EstimateStructure(refine, only_unestimated); }
        return structure_dict(st, e.options_.bundle_adjust_tracks, refine);
      }, py::arg("refine") = false, py::arg("only_unestimated") = false)
      // the reference returns its BundleAdjustmentSummary: the LastBundleAdjustmentSummary() dict plus success and num_points_removed
      .def("BundleAdjustmentAndRemoveOutlierPoints", [](GlobalReconstructionEstimator& e) {
        bool ok;
        { py::gil_scoped_release release; ok = e.BundleAdjustmentAndRemoveOutlierPoints(); }
        py::dict d = bundle_dict(e.bundle_);
        d["success"] = ok; d["num_points_removed"] = e.outlier_.num_removed;
        return d;
      })
      .def("LastOutlierSummary", [](const GlobalReconstructionEstimator& e) { return outlier_dict(e.outlier_); })
      .def("BundleAdjustCameraPositionsAndPoints", &GlobalReconstructionEstimator::BundleAdjustCameraPositionsAndPoints,
           py::call_guard<py::gil_scoped_release>())
      .def("BundleAdjustment", &GlobalReconstructionEstimator::BundleAdjustment, py::call_guard<py::gil_scoped_release>())
      .def("LastBundleAdjustmentSummary", [](const GlobalReconstructionEstimator& e) { return bundle_dict(e.bundle_); })
      // the track selection of the last bundle adjustment, either kind: ran (false when subsample_tracks_for_bundle_adjustment is unset), the
      // six counts of gsfm_tracks_select_good by name, the three parameters, kernel_ms
      .def("LastTrackSelection", [](const GlobalReconstructionEstimator& e) { return selection_dict(e.selection_); })
      .def("LastStructureSummary", [](const GlobalReconstructionEstimator& e) { return structure_dict(e.structure_, e.options_.bundle_adjust_tracks, e.structure_refine_asked_); })
      .def("LastSummary", [](const GlobalReconstructionEstimator& e) { return summary_dict(e.summary_); })
      .def("LastError", [](const GlobalReconstructionEstimator& e) { return e.error_; });

  m.def("Read1DSFM", [](const std::string& dir, Reconstruction* rec, ViewGraph* vg, CovarianceMap& cov) {  // bind :611-617
    std::string err;
    if (!gsfm::Read1DSFMViewGraph(dir, vg, &err)) throw std::runtime_error(err);
    for (ViewId v : vg->ViewIds()) rec->views.insert(v);
    gsfm::Tracks1DSfM tracks;
    if (gsfm::Read1DSFMTracks(dir, &tracks, nullptr)) {  // keypoints + tracks, when the dataset has them
      auto em = std::make_shared<gsfm::EdgeMatches>();
      gsfm::CollectEdgeMatches(tracks, *vg, em.get());
      rec->matches = em;
      for (const auto& kv : tracks.names) if (rec->views.count(kv.first)) rec->view_names[kv.first] = kv.second;
      rec->track_point.clear();
      rec->track_estimated.clear();
      rec->tracks = std::make_shared<gsfm::Tracks1DSfM>(std::move(tracks));   // kept for EstimateStructure()
    }
    for (ViewId v : rec->views) if (!rec->view_names.count(v)) rec->view_names[v] = std::to_string(v);  // no list.txt: the id is the name
    gsfm::ReadCovariance(dir, &cov);
  });
  py::class_<FeaturesAndMatchesDatabase>(m, "FeaturesAndMatchesDatabase").def(py::init([](const std::string& p) { return new FeaturesAndMatchesDatabase{p}; }));
  // src/read_colmap_posegraph.cpp:55-164
  m.def("AddColmapMatchesToReconstructionBuilder", [](const std::string& two_views, const std::string& images_wildcard, ReconstructionBuilder* b) {
    gsfm::ColmapPoseGraph g;
    std::string err;
    if (!gsfm::ReadColmapTwoViews(two_views, gsfm::ExpandWildcard(images_wildcard), &g, &err)) throw std::runtime_error(err);
    for (const auto& e : g.view_graph.GetAllEdges()) b->view_graph->AddEdge(e.first.first, e.first.second, e.second);
    for (size_t v = 0; v < g.view_names.size(); ++v) { b->reconstruction->views.insert((ViewId)v); b->reconstruction->view_names[(ViewId)v] = g.view_names[v]; }
    b->reconstruction->matches = std::make_shared<gsfm::EdgeMatches>(std::move(g.matches));
  });
  // bind :286-287 -> src/uncertainty.cpp:164-198; returns the counters (the reference returns None)
  m.def("store_covariance_rot", [](const std::string& dir, Reconstruction* rec, ViewGraph* vg) {
    if (!rec->matches) throw std::runtime_error("store_covariance_rot: the reconstruction carries no matched features (dataset without tracks)");
    gsfm::CalcCovarianceStats st;
    std::string err;
    {
      py::gil_scoped_release release;
      if (!gsfm::StoreCovarianceRot(dir, *rec->matches, *vg, nullptr, &st, &err)) { py::gil_scoped_acquire a; throw std::runtime_error(err); }
    }
    py::dict d;
    d["num_edges"] = st.num_edges; d["num_matches"] = st.num_matches; d["num_written"] = st.num_written;
    d["num_skipped"] = st.num_skipped; d["num_singular"] = st.num_singular; d["kernel_ms"] = st.kernel_ms;
    return d;
  });
  m.def("ReadCovariance", [](const std::string& dir, CovarianceMap& cov) { gsfm::ReadCovariance(dir, &cov); });
  m.def("WriteCovariance", [](const std::string& dir, const CovarianceMap& cov) { return gsfm::WriteCovariance(dir, cov); });
  // The flattened inputs CalcCovariance hands to gsfm_cov_estimate, for inspection and for globalsfmpy_amd.covariance.
  m.def("Read1DSFMEdgeMatches", [](const std::string& dir) {
    gsfm::Tracks1DSfM tracks;
    theia::ViewGraph vg;
    std::string err;
    if (!gsfm::Read1DSFMTracks(dir, &tracks, &err) || !gsfm::Read1DSFMViewGraph(dir, &vg, &err)) throw std::runtime_error(err);
    gsfm::EdgeMatches em;
    gsfm::CollectEdgeMatches(tracks, vg, &em);
    return edge_matches_dict(em);
  });
  // bind :623-628: estimates every edge's rotation covariance on the device and writes <dir>/covariance_rot.txt;
  // returns the counters (the reference returns None).
  m.def("CalcCovariance", [](const std::string& dir) {
    gsfm::CalcCovarianceStats st;
    std::string err;
    {
      py::gil_scoped_release release;
      if (!gsfm::CalcCovariance(dir, nullptr, &st, &err)) { py::gil_scoped_acquire a; throw std::runtime_error(err); }
    }
    py::dict d;
    d["num_edges"] = st.num_edges; d["num_matches"] = st.num_matches; d["num_written"] = st.num_written;
    d["num_skipped"] = st.num_skipped; d["num_singular"] = st.num_singular; d["kernel_ms"] = st.kernel_ms;
    return d;
  });
  m.def("OrientationsFromMaximumSpanningTree", [](const ViewGraph& vg, OrientationMap* o) { return OrientationsFromMaximumSpanningTree(vg, o); });
  m.def("OrientationsFromMaximumSpanningTreeOnDevice", [](const ViewGraph& vg, OrientationMap* o) { return OrientationsFromMaximumSpanningTreeOnDevice(vg, o); });
  m.def("FilterViewPairsFromOrientation", &FilterViewPairsFromOrientation);
  py::class_<FilterViewPairsFromRelativeTranslationOptions>(m, "FilterViewPairsFromRelativeTranslationOptions")
      .def(py::init<>())
      .def_readwrite("num_threads", &FilterViewPairsFromRelativeTranslationOptions::num_threads)
      .def_readwrite("num_iterations", &FilterViewPairsFromRelativeTranslationOptions::num_iterations)
      .def_readwrite("translation_projection_tolerance", &FilterViewPairsFromRelativeTranslationOptions::translation_projection_tolerance)
      .def_readwrite("seed", &FilterViewPairsFromRelativeTranslationOptions::seed);
  m.def("FilterViewPairsFromRelativeTranslation", &FilterViewPairsFromRelativeTranslation, py::call_guard<py::gil_scoped_release>());
  // the reference binds neither this function nor its input; here the matches are those the reconstruction carries
  m.def("RefineRelativeTranslationsWithKnownRotations", [](const Reconstruction& rec, const OrientationMap& o, int num_threads, ViewGraph* vg) {
    if (!rec.matches) throw std::runtime_error("RefineRelativeTranslationsWithKnownRotations: the reconstruction carries no matched features");
    RefineRelativeTranslationsStats st;
    { py::gil_scoped_release release; st = RefineRelativeTranslationsWithKnownRotations(*rec.matches, o, num_threads, vg); }
    return refine_stats_dict(st);
  });
  // bind :658, src/compare_reconstructions.cpp:617-647: (view_graph, reconstruction_to_eval, covariances, residuals) -- fills `residuals`
  m.def("residuals_of_relative_rot", [](const ViewGraph& vg, const Reconstruction& rec, const CovarianceMap& cov, std::vector<double>& residuals) {
    gsfm::ResidualsOfRelativeRotations(vg, rec.orientation, cov, &residuals);
  }, py::call_guard<py::gil_scoped_release>());
  m.def("SetOrientations", [](const OrientationMap& o, Reconstruction* rec) {  // bind :80-98
    rec->orientation.clear();
    for (const auto& kv : o) if (rec->views.count(kv.first)) rec->orientation[kv.first] = kv.second;
  });
  // bind :273 (Theia's SetReconstructionFromEstimatedPoses): the orientation and, where there is
  // one, the position of every view of the reconstruction that has an estimated orientation
  m.def("SetReconstructionFromEstimatedPoses", [](const OrientationMap& o, const OrientationMap& p, Reconstruction* rec) {
    rec->orientation.clear();
    rec->position.clear();
    for (const auto& kv : o) {
      if (!rec->views.count(kv.first)) continue;
      rec->orientation[kv.first] = kv.second;
      auto it = p.find(kv.first);
      if (it != p.end()) rec->position[kv.first] = it->second;
    }
  }, py::call_guard<py::gil_scoped_release>());
  m.def("InitGlog", [](int, bool, std::string) {}, py::arg("log_level") = 0, py::arg("logtostderr") = true, py::arg("log_dir") = "./log");
  m.def("StopGlog", []() {});
  m.def("WriteReconstruction", [](const Reconstruction& rec, const std::string& path) {
    std::ofstream f(path);
    f << "# view_id angle_axis(3)  -- rotation-only reconstruction written by the MI355X build\n";
    for (const auto& kv : rec.orientation) f << kv.first << " " << kv.second[0] << " " << kv.second[1] << " " << kv.second[2] << "\n";
    return (bool)f;
  });
  // bind :631 / Theia io/write_ply_file.cc:74-123: the estimated tracks' points, then the positions of the estimated views as green
  // vertices (gsfm::WritePlyFile).  Without an estimated track the file holds the views alone.
  // Theia's SetUnderconstrainedAsUnestimated; returns the counters (the reference returns None)
  m.def("SetUnderconstrainedAsUnestimated", [](Reconstruction* rec) {
    const gsfm::UnderconstrainedStats st = gsfm::SetUnderconstrainedAsUnestimated(rec);
    py::dict d;
    d["rounds"] = st.rounds; d["views_removed"] = st.views_removed; d["tracks_removed"] = st.tracks_removed;
    return d;
  });
  // Theia's SelectGoodTracksForBundleAdjustment with its argument order; the chosen track ids as a sorted list where Theia fills an unordered_set
  m.def("SelectGoodTracksForBundleAdjustment", [](const Reconstruction& rec, int long_track_length_threshold, int image_grid_cell_size_pixels,
                                                  int min_num_optimized_tracks_per_view) {
    std::vector<uint8_t> subset;
    {
      py::gil_scoped_release release;
      gsfm::SelectGoodTracksForBundleAdjustment(rec, long_track_length_threshold, image_grid_cell_size_pixels, min_num_optimized_tracks_per_view, &subset);
    }
    std::vector<uint64_t> ids;
    for (size_t t = 0; t < subset.size(); ++t) if (subset[t]) ids.push_back(t);
    return ids;
  }, py::arg("reconstruction"), py::arg("long_track_length_threshold") = 10, py::arg("image_grid_cell_size_pixels") = 100,
  py::arg("min_num_optimized_tracks_per_view") = 200);
  // Theia's SetOutlierTracksToUnestimated, its name, argument order and return value (the number of tracks removed)
  m.def("SetOutlierTracksToUnestimated", [](double max_inlier_reprojection_error, double min_triangulation_angle_degrees, Reconstruction* rec) {
    return (int)gsfm::SetOutlierTracksToUnestimated(max_inlier_reprojection_error, min_triangulation_angle_degrees, rec).num_removed;
  }, py::call_guard<py::gil_scoped_release>());
  m.def("WritePlyFile", [](const std::string& ply_file, const Reconstruction& rec, int min_num_observations_per_point) {
    if (ply_file.empty()) throw std::invalid_argument("WritePlyFile: empty file name");
    return gsfm::WritePlyFile(ply_file, rec, min_num_observations_per_point);
  }, py::call_guard<py::gil_scoped_release>());
  // ---- evaluation (bind :387-394, :396-403, :651-664; orientations only) ----
  py::class_<gsfm::CompareInfo>(m, "CompareInfo")
      .def(py::init<>())
      .def_readwrite("rotation_diff_when_align", &gsfm::CompareInfo::rotation_diff_when_align)
      .def_readwrite("position_errors", &gsfm::CompareInfo::position_errors)
      .def_readwrite("num_3d_points", &gsfm::CompareInfo::num_3d_points)
      .def_readwrite("common_camera", &gsfm::CompareInfo::common_camera)
      .def_readwrite("num_reconstructed_view", &gsfm::CompareInfo::num_reconstructed_view);
  py::class_<gsfm::ColmapViewGraph>(m, "ColmapViewGraph")
      .def(py::init<>())
      .def("read_poses", &gsfm::ColmapViewGraph::read_poses)
      .def_readwrite("num_view", &gsfm::ColmapViewGraph::num_view)
      .def_readwrite("image_ids", &gsfm::ColmapViewGraph::image_ids)
      .def_readwrite("image_names", &gsfm::ColmapViewGraph::image_names)
      .def_readwrite("poses", &gsfm::ColmapViewGraph::poses);
  m.def("AngularDifference", &gsfm::AngularDifference);
  m.def("AlignRotations", [](const std::vector<Eigen::Vector3d>& gt, std::vector<Eigen::Vector3d> rot) {
    const gsfm::AlignmentSummary s = gsfm::AlignRotations(gt, &rot);
    py::dict d;
    d["alignment"] = s.alignment; d["initial_cost"] = s.initial_cost; d["final_cost"] = s.final_cost;
    d["iterations"] = s.iterations; d["converged"] = s.converged; d["message"] = s.message;
    return py::make_tuple(rot, d);
  }, "Returns (aligned rotations, summary); the reference aligns in place.");
  m.def("FindCommonViewsByName", &gsfm::FindCommonEstimatedViewsByName);
  m.def("FindCommonViewsByNameColmap", &gsfm::FindCommonEstimatedViewsByNameColmap);
  m.def("compare_orientations", &gsfm::compare_orientations);
  m.def("compare_orientations_colmap", &gsfm::compare_orientations_colmap);
  m.def("ReadImageSize", [](const std::string& path) {
    int w = 0, h = 0;
    if (!gsfm::ReadImageSize(path, &w, &h)) throw std::runtime_error("cannot read the size of image " + path);
    return py::make_tuple(w, h);
  });
  m.def("tgamma", [](double x) { return std::tgamma(x); });

  // gamma constants / tables (bind :663-686), regenerated by the library
  for (int nu : {3, 4, 9}) {
    const std::string s = std::to_string(nu);
    double C, q, gk;
    gsfm_magsac_constants(nu, &C, &q, &gk);
    const int n = gsfm_magsac_table(nu, nullptr, 0);
    std::vector<double> t(n);
    gsfm_magsac_table(nu, t.data(), n);
    m.attr(("nu" + s).c_str()) = py::float_((double)nu);
    m.attr(("stored_gamma_values" + s).c_str()) = py::cast(t);
    m.attr(("C" + s).c_str()) = py::float_(C);
    m.attr(("sigma_quantile" + s).c_str()) = py::float_(q);
    m.attr(("upper_incomplete_gamma_of_k" + s).c_str()) = py::float_(gk);
    m.attr(("stored_gamma_number" + s).c_str()) = py::int_(n);
    m.attr(("precision_of_stored_gamma" + s).c_str()) = py::float_(1000.0);
  }
}
