// The callers and data formats either side of the hot path ("next" rows of SURVEY section 8f),
// host-side C++: a minimal theia::ViewGraph, the maximum-spanning-tree initialisation, the 1DSfM
// EGs.txt / covariance_rot.txt codecs, the post-rotation edge filter and the evaluation metrics.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <memory>

#include "compat.hpp"

namespace gsfm { struct EdgeMatches; struct Tracks1DSfM; struct TrackBuildStats; }

namespace theia {

// Subset of thirdparty/TheiaSfM/src/theia/sfm/view_graph/view_graph.h used around the rotation path.
class ViewGraph {
 public:
  int NumViews() const { return (int)vertices_.size(); }
  int NumEdges() const { return (int)edges_.size(); }
  bool HasView(ViewId v) const { return vertices_.count(v) != 0; }
  bool HasEdge(ViewId a, ViewId b) const { return edges_.count(Key(a, b)) != 0; }
  std::unordered_set<ViewId> ViewIds() const;
  // The key is normalised to (min, max); the payload is stored untouched (view_graph.cc:133-153).
  void AddEdge(ViewId a, ViewId b, const TwoViewInfo& info);
  bool RemoveEdge(ViewId a, ViewId b);
  bool RemoveView(ViewId v);
  const TwoViewInfo* GetEdge(ViewId a, ViewId b) const;
  TwoViewInfo* GetMutableEdge(ViewId a, ViewId b);
  const std::unordered_set<ViewId>* GetNeighborIdsForView(ViewId v) const;
  const std::unordered_map<ViewIdPair, TwoViewInfo>& GetAllEdges() const { return edges_; }
  void GetLargestConnectedComponentIds(std::unordered_set<ViewId>* out) const;
  void ExtractSubgraph(const std::unordered_set<ViewId>& keep, ViewGraph* sub) const;
  static ViewIdPair Key(ViewId a, ViewId b) { return a < b ? ViewIdPair(a, b) : ViewIdPair(b, a); }

 private:
  std::unordered_map<ViewId, std::unordered_set<ViewId>> vertices_;
  std::unordered_map<ViewIdPair, TwoViewInfo> edges_;
};

#ifndef GSFM_USE_REAL_THEIA
// Only what the rotation stage reads/writes of a theia::Reconstruction: the set of views and the
// estimated orientation per view (SetOrientations, bind_src/GlobalSfMpy.cpp:80-98). Tracks, cameras and
// intrinsics are out of scope.
class Reconstruction {
 public:
  std::unordered_map<ViewId, Eigen::Vector3d> orientation;
  std::unordered_map<ViewId, Eigen::Vector3d> position;   // estimated camera positions (SetReconstructionFromEstimatedPoses)
  std::unordered_set<ViewId> views;
  std::unordered_map<ViewId, std::string> view_names;  // COLMAP ingestion: image file name per view
  // The matched features of the view pairs, in place of theia's tracks: all that store_covariance_rot reads of them
  // (get_matched_features, src/uncertainty.cpp:3-33).  Set by Read1DSFM (when tracks.txt exists) and by
  // AddColmapMatchesToReconstructionBuilder.
  std::shared_ptr<const gsfm::EdgeMatches> matches;
  // The keypoints and tracks of a 1DSfM dataset (Read1DSFM, when tracks.txt exists), and per track of them what EstimateStructure
  // stored: the triangulated point and whether the track is estimated (both empty until then).
  std::shared_ptr<const gsfm::Tracks1DSfM> tracks;
  std::vector<Eigen::Vector3d> track_point;
  std::vector<uint8_t> track_estimated;
  // The estimated focal length per view, in pixels: empty until a bundle adjustment with free focal lengths writes it (BundleAdjustment with
  // FOCAL_LENGTH).  FlattenTracks takes a view's entry in place of the EXIF / 1.2 x rule, so every later call sees the adjusted value.
  std::unordered_map<ViewId, double> focal_length;
  // What the track builder reported when CheckView() built the tracks from the matches (the COLMAP branch); empty otherwise.
  std::shared_ptr<const gsfm::TrackBuildStats> track_build;
  int NumTracks() const;
  int NumEstimatedTracks() const;
  int NumViews() const { return (int)views.size(); }
};
#endif

// thirdparty/TheiaSfM/src/theia/sfm/view_graph/orientations_from_maximum_spanning_tree.cc:109-181
bool OrientationsFromMaximumSpanningTree(const ViewGraph& view_graph, std::unordered_map<ViewId, Eigen::Vector3d>* orientations);
// The same initialisation on the device (gsfm_rot_init_spanning_tree): the edges flattened in sorted ViewIdPair order with dense
// index = rank of the ViewId, so that the device's tie-break (weight desc, edge index asc) is theia's (weight desc, first asc, second
// asc) and both choose the same tree.  Fills the orientations of the tree component only, like the host function; returns false for
// an empty graph; throws std::runtime_error when no device is usable (there is no CPU fallback) or the device call fails.
bool OrientationsFromMaximumSpanningTreeOnDevice(const ViewGraph& view_graph, std::unordered_map<ViewId, Eigen::Vector3d>* orientations);

// thirdparty/TheiaSfM/src/theia/sfm/filter_view_pairs_from_orientation.cc:55-122: drops the edges whose
// relative rotation disagrees with the global orientations by more than the threshold (and the edges touching a view
// without an orientation).  The angles of all edges are one device sweep (gsfm_rot_edge_sq_norms); throws
// std::runtime_error when no device is usable (there is no CPU fallback).
void FilterViewPairsFromOrientation(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                    double max_relative_rotation_difference_degrees, ViewGraph* view_graph);
// thirdparty/TheiaSfM/src/theia/sfm/filter_view_pairs_from_relative_translation.h: the 1DSfM filter of relative translations.
struct FilterViewPairsFromRelativeTranslationOptions {
  int num_threads = 1;                              // accepted and ignored: the projections run side by side on the device
  int num_iterations = 48;                          // number of random projection axes
  double translation_projection_tolerance = 0.08;   // an edge goes when its summed bad weight exceeds this times num_iterations
  uint64_t seed = 1;                                // in place of the reference's rng pointer: seeds the library's own axis generator
};
// filter_view_pairs_from_relative_translation.cc:256-308 on the device (gsfm_pos_filter_relative_translations, under the reproducible
// definition of include/gsfm_pos.h: the library's own axes, integer arc weights, the smallest index among equal scores).  The edges are
// flattened in sorted ViewIdPair order with dense index = rank of the ViewId among the graph's views.  An edge whose first view has no
// orientation is skipped and kept (the reference aborts in FindOrDie).  Throws std::runtime_error when no device is usable (there is no
// CPU fallback) or the device call fails.
void FilterViewPairsFromRelativeTranslation(const FilterViewPairsFromRelativeTranslationOptions& options,
                                            const std::unordered_map<ViewId, Eigen::Vector3d>& orientations, ViewGraph* view_graph);
// thirdparty/TheiaSfM/src/theia/sfm/reconstruction_estimator_utils.cc:244-269 -> optimize_relative_position_with_known_rotation.cc on the
// device (gsfm_pos_refine_relative_translations, under the definition of include/gsfm_pos.h): every edge of the view graph that has
// matches in `matches` and whose two views both have an orientation gets its position_2 replaced by the refined unit vector.  Any other
// edge keeps its position_2 (the reference reads the matches from the reconstruction's tracks and aborts in FindOrDie on a missing
// orientation), and so does an edge with fewer than 2 matches (skipped) or a non-finite result.  num_threads is accepted and ignored: the
// edges run side by side on the device, one wavefront each.  Throws std::runtime_error when no device is usable (there is no CPU
// fallback) or the device call fails.
struct RefineRelativeTranslationsStats {
  size_t num_refined = 0, num_skipped = 0, num_nonfinite = 0;
  double kernel_ms = 0.0;
};
RefineRelativeTranslationsStats RefineRelativeTranslationsWithKnownRotations(const gsfm::EdgeMatches& matches,
                                                                             const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                                             int num_threads, ViewGraph* view_graph);
// thirdparty/TheiaSfM/src/theia/sfm/view_graph/remove_disconnected_view_pairs.cc: keeps the largest component.
std::unordered_set<ViewId> RemoveDisconnectedViewPairs(ViewGraph* view_graph);

}  // namespace theia

namespace gsfm {
// 1DSfM: EGs.txt (+ cc.txt restriction) -> view graph. Convention of io/read_1dsfm.cc:299-372:
// R' = S R^T S with S = diag(1,-1,-1), no re-orthonormalisation, t' = S t.  When tracks.txt / coords.txt / list.txt are
// present, num_verified_matches = number of common tracks and the focal lengths follow read_1dsfm.cc:341-362.
bool Read1DSFMViewGraph(const std::string& dataset_directory, theia::ViewGraph* view_graph, std::string* error);
void AnnotateViewGraphFromTracks(const std::string& dataset_directory, theia::ViewGraph* view_graph);
// covariance_rot.txt codec (src/uncertainty.cpp:164-230): doubles stored as the decimal of their bit pattern.
bool ReadCovariance(const std::string& dataset_directory, CovarianceMap* covariances);
bool WriteCovariance(const std::string& dataset_directory, const CovarianceMap& covariances);

// ---- 1DSfM keypoints and tracks + the CalcCovariance driver ----
// What thirdparty/TheiaSfM/src/theia/io/read_1dsfm.cc:114-292 reads besides the epipolar geometries: list.txt (view id =
// line index, optional EXIF focal), coords.txt (per view: principal point, keypoints) and tracks.txt.
struct Tracks1DSfM {
  std::unordered_map<theia::ViewId, double> focal;  // list.txt; 0 = no EXIF focal (read_1dsfm.cc:136-142)
  std::unordered_map<theia::ViewId, std::string> names;  // list.txt: file name without its directory (:128-130)
  std::unordered_map<theia::ViewId, Eigen::Vector2d> principal_point;  // coords.txt header (parsed as float, :176-193)
  std::unordered_map<theia::ViewId, std::vector<Eigen::Vector2d>> keypoints;
  std::vector<std::vector<std::pair<theia::ViewId, int>>> tracks;  // (view, keypoint index)
};
bool Read1DSFMTracks(const std::string& dataset_directory, Tracks1DSfM* out, std::string* error);

// The matched features of every view-graph edge, flattened for gsfm_cov_estimate: the common tracks of the two views
// (get_matched_features, src/uncertainty.cpp:3-33), the intrinsics of :99-104 and TwoViewInfo::rotation_2/position_2.
struct EdgeMatches {
  std::vector<theia::ViewIdPair> edges;  // sorted by key
  std::vector<uint64_t> match_ptr;       // edges.size() + 1
  std::vector<double> matches;           // x1 y1 x2 y2
  std::vector<double> intrinsics;        // f1 u1 v1 f2 u2 v2
  std::vector<double> rotation, position;
  // COLMAP ingestion only: per view the focal length of the first two_views.txt line that names it
  std::unordered_map<theia::ViewId, double> first_focal;
};
void CollectEdgeMatches(const Tracks1DSfM& tracks, const theia::ViewGraph& view_graph, EdgeMatches* out);

// ---- Tracks from the matches (the COLMAP branch: src/GSfM_reconstruction_builder.cpp:423-444 -> Theia's TrackBuilder), on the device:
// gsfm_tracks_build under the definition of include/gsfm_tracks.h ----
// Every match of `matches` is one AddFeatureCorrespondence, in the order of the flattened arrays (edges by sorted ViewIdPair, an edge's matches
// as listed); dense view index = rank of the ViewId among the views the edges name.  Fills `out` as Read1DSFMTracks fills it for a 1DSfM dataset:
// keypoints per view = the view's features that a track kept, in feature-id order; tracks as (view, keypoint index) in the entry's order; focal =
// EdgeMatches::first_focal where it has the view, else that of the first edge naming it; principal point = that of the first edge naming the view.
// names stay empty (the caller has them).  Throws when matches exist and no device is usable (NoDeviceError: there is no CPU fallback) or the
// device call fails (std::runtime_error).
struct NoDeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct TrackBuildStats {
  bool built = false;            // CheckView(): false when no device was usable; `error` then says why and the reconstruction has no tracks
  std::string error;
  size_t num_matches = 0, num_tracks = 0, num_observations = 0;
  uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};   // features, components, small, inconsistent, degenerate, replayed, tracks
  int min_track_length = 2, max_track_length = 1000;
  double kernel_ms = 0.0;
};
TrackBuildStats BuildTracksFromMatches(const EdgeMatches& matches, int min_track_length, int max_track_length, Tracks1DSfM* out);

#ifndef GSFM_USE_REAL_THEIA
// ---- EstimateStructure without the per-track refinement (src/GSfM_global_reconstruction_estimator.cpp:621-636 -> Theia's
// TrackEstimator with bundle_adjustment = false), on the device: gsfm_tracks_triangulate under the definition of include/gsfm_tracks.h ----
// The reconstruction's tracks as that entry point takes them.  Cameras: every view that has keypoints, ascending by view id; a camera is
// estimated when the reconstruction holds an orientation AND a position for it (SetReconstructionFromEstimatedPoses), others carry zeros.
// Intrinsics f u v: the reconstruction's estimated focal length of the view when it has one (Reconstruction::focal_length), else the EXIF
// focal of list.txt, else 1.2 x the principal point's x (the rule of CollectEdgeMatches), and the principal point of coords.txt.  Tracks and their observations in the order of tracks.txt.
struct FlatTracks {
  std::vector<theia::ViewId> views;                  // camera index -> view id
  std::vector<double> rot_aa, cam_pos, intrinsics;   // 3 per camera
  std::vector<uint8_t> cam_estimated;
  std::vector<uint64_t> track_ptr;
  std::vector<uint32_t> obs_cam;
  std::vector<double> obs_xy;
};
void FlattenTracks(const theia::Reconstruction& reconstruction, FlatTracks* out);
// The sub-CSR of the tracks that are NOT estimated (track_estimated 0 or not yet set), in ascending track order: track_ptr, obs_cam and obs_xy
// of `out` are replaced by those tracks' slices, the cameras stay; track_index[k] is the track the sub-batch's k-th track is.  Host code.
void KeepUnestimatedTracks(const theia::Reconstruction& reconstruction, FlatTracks* out, std::vector<uint64_t>* track_index);
struct EstimateStructureStats {
  size_t num_tracks = 0, num_estimated = 0;
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};           // tracks per status of gsfm_tracks_triangulate
  double kernel_ms = 0.0;
  // the refined call (gsfm_tracks_triangulate_refine) only
  bool tracks_refined = false;
  uint64_t num_refinement_failed = 0;                // status 6
  double mean_iterations = 0.0;                      // over the refined tracks
  int max_iterations = 0;
};
// The per-track refinement EstimateStructure may run (Theia's BundleAdjustTrack under the definition of include/gsfm_tracks.h): the loss
// as BundleAdjustmentOptions names it (TRIVIAL, HUBER, SOFTLONE; anything else throws std::runtime_error) and its width.
struct TrackRefinement {
  std::string loss_function = "TRIVIAL";
  double loss_width = 10.0;
  int max_num_iterations = 100;
};
// One call of gsfm_tracks_triangulate -- with `refinement`, of gsfm_tracks_triangulate_refine -- over all tracks; stores point and estimated flag per track in the reconstruction.  A reconstruction
// without tracks is left alone.  Throws std::runtime_error when no device is usable (there is no CPU fallback) or the device call fails.
// only_unestimated (Theia's TrackEstimator::EstimateTracks, which skips the estimated tracks): the same entry runs on KeepUnestimatedTracks'
// sub-batch and its points and flags are scattered back by index; an estimated track keeps its point bytes and its flag, and the stats
// count the sub-batch.  The entry's permutation guarantee makes a track's result that of a call over all tracks.
EstimateStructureStats EstimateStructure(double min_triangulation_angle_degrees, double max_reprojection_error_pixels,
                                         theia::Reconstruction* reconstruction, const TrackRefinement* refinement = nullptr,
                                         bool only_unestimated = false);
// Theia's SetOutlierTracksToUnestimated (sfm/set_outlier_tracks_to_unestimated.cc) on the device: gsfm_tracks_outlier_tracks under the
// definition of include/gsfm_tracks.h, over FlattenTracks' arrays plus track_point / track_estimated.  Clears the flag of every track of
// status 2, 3 or 4 and leaves track_point alone, as Theia leaves the point.  num_removed is Theia's return value.  A reconstruction without
// tracks is left alone.  Throws std::runtime_error when no device is usable (there is no CPU fallback) or the device call fails.
struct OutlierTracksStats {
  size_t num_examined = 0;                           // tracks estimated on input
  uint64_t counts[5] = {0, 0, 0, 0, 0};              // tracks per status of gsfm_tracks_outlier_tracks
  size_t num_removed = 0;                            // counts[2] + counts[3] + counts[4]
  double kernel_ms = 0.0;
};
OutlierTracksStats SetOutlierTracksToUnestimated(double max_reprojection_error_pixels, double min_triangulation_angle_degrees,
                                                 theia::Reconstruction* reconstruction);
// Theia's io/write_ply_file.cc: the points of the estimated tracks with at least min_num_observations_per_point views (no colour: 0 0 0;
// ascending track index where Theia walks a hash set), then the estimated views' positions in green.  A view without a position is
// written at the origin (a rotation-only reconstruction).  Returns false when the file cannot be written.
bool WritePlyFile(const std::string& ply_file, const theia::Reconstruction& reconstruction, int min_num_observations_per_point);

// Theia's SetUnderconstrainedAsUnestimated (sfm/set_underconstrained_as_unestimated.cc), the step before the bundle adjustment: estimated
// views that see fewer than 3 estimated tracks become unestimated (their orientation and position leave the reconstruction), then
// estimated tracks seen by fewer than 2 estimated views become unestimated; both passes alternate until either changes nothing.  A view is
// estimated when the reconstruction holds an orientation and a position for it (FlattenTracks' rule).  Host code.
struct UnderconstrainedStats {
  int rounds = 0, views_removed = 0, tracks_removed = 0;
};
UnderconstrainedStats SetUnderconstrainedAsUnestimated(theia::Reconstruction* reconstruction);

// GlobalReconstructionEstimator::BundleAdjustCameraPositionsAndPoints (src/GSfM_global_reconstruction_estimator.cpp -> Theia's
// BundleAdjuster with fixed orientations and intrinsics) on the device: gsfm_ba_solve under the definition of include/gsfm_ba.h, over
// FlattenTracks' arrays plus track_estimated / track_point.  Writes the positions of the estimated views and the points of the estimated
// tracks back.  usable: Ceres' IsSolutionUsable (every termination but FAILURE).  The loss as BundleAdjustmentOptions names it (TRIVIAL,
// HUBER, SOFTLONE; anything else throws std::runtime_error).  A reconstruction without tracks is left alone (usable, ran = false).
struct BundleAdjustmentStats {
  bool ran = false, usable = true;
  int termination = -1, num_iterations = 0, num_successful_steps = 0, num_unsuccessful_steps = 0, num_cg_iterations = 0, max_num_iterations = 0;
  uint64_t num_observations = 0, num_cameras = 0, num_points = 0;
  double initial_cost = 0.0, final_cost = 0.0, t_total_ms = 0.0;
  bool focal_lengths_free = false;                   // BundleAdjustment with FOCAL_LENGTH
};
// tracks_to_optimize (Theia's SelectGoodTracksForBundleAdjustment, below): one byte per track; the solver's point_estimated is
// track_estimated AND tracks_to_optimize, and only those points are written back.  NULL: every estimated track, today's call byte for byte.
BundleAdjustmentStats BundleAdjustCameraPositionsAndPoints(const std::string& loss_function, double loss_width, int max_num_iterations,
                                                           theia::Reconstruction* reconstruction,
                                                           const std::vector<uint8_t>* tracks_to_optimize = nullptr);
// Theia's SelectGoodTracksForBundleAdjustment (sfm/select_good_tracks_for_bundle_adjustment.cc) on the device: gsfm_tracks_select_good under
// the definition of include/gsfm_tracks.h, over FlattenTracks' arrays plus track_point / track_estimated.  tracks_to_optimize gets one byte
// per track: 0, 1 (selected by a grid cell) or 2 (by the top-up).  Nothing in the reconstruction changes.  A reconstruction without tracks
// gives an empty vector (ran = false).  Throws std::runtime_error when no device is usable (there is no CPU fallback), an argument is
// refused or the device call fails.
struct TrackSelectionStats {
  bool ran = false;
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};   // tracks with items, cells, selected by a cell, cameras topped up, selected by the top-up, selected
  int long_track_length_threshold = 0, image_grid_cell_size_pixels = 0, min_num_optimized_tracks_per_view = 0;
  uint64_t num_deficient_items = 0;          // what the host downloaded for the top-up
  double kernel_ms = 0.0, replay_ms = 0.0;
};
TrackSelectionStats SelectGoodTracksForBundleAdjustment(const theia::Reconstruction& reconstruction, int long_track_length_threshold,
                                                        int image_grid_cell_size_pixels, int min_num_optimized_tracks_per_view,
                                                        std::vector<uint8_t>* tracks_to_optimize);
// Theia's OptimizeIntrinsicsType (sfm/bundle_adjustment/bundle_adjustment.h): a bitmask, with Theia's names and values.
// (unscoped, so that values combine with | as Theia's do; in a namespace of its own to keep NONE and ALL out of gsfm)
namespace optimize_intrinsics {
enum Type : int {
  NONE = 0x00, FOCAL_LENGTH = 0x01, ASPECT_RATIO = 0x02, SKEW = 0x04, PRINCIPAL_POINTS = 0x08, RADIAL_DISTORTION = 0x10, TANGENTIAL_DISTORTION = 0x20,
  ALL = 0x3f
};
}
using OptimizeIntrinsicsType = optimize_intrinsics::Type;
// The flag string of the reference's StringToOptimizeIntrinsicsType: names joined by '|' without spaces; a first name of NONE or ALL decides
// alone.  false (and *error) for an empty string or a name that is none of the enum's -- the reference aborts there.
bool ParseOptimizeIntrinsicsType(const std::string& text, int* mask, std::string* error);
// the names of the mask's bits joined by '|' (NONE for 0)
std::string OptimizeIntrinsicsTypeNames(int mask);
// GlobalReconstructionEstimator::BundleAdjustment (the solve of BundleAdjustmentAndRemoveOutlierPoints) on the device, over all estimated views
// and tracks.  As above, and the orientations of the estimated views are written back as well.  intrinsics_to_optimize:
//   NONE          gsfm_ba6_solve under the definition of include/gsfm_ba6.h: the intrinsics FlattenTracks gives are held;
//   FOCAL_LENGTH  gsfm_ba7_solve under the definition of include/gsfm_ba7.h: the focal length of every estimated view moves too, from the
//                 value FlattenTracks gives, and is written to Reconstruction::focal_length (stats.focal_lengths_free);
//   any other bit throws std::invalid_argument naming the unsupported bits before any device call: the reconstruction is untouched.
//   tracks_to_optimize: as for BundleAdjustCameraPositionsAndPoints.
BundleAdjustmentStats BundleAdjustment(const std::string& loss_function, double loss_width, int max_num_iterations, int intrinsics_to_optimize,
                                       theia::Reconstruction* reconstruction, const std::vector<uint8_t>* tracks_to_optimize = nullptr);
#endif

// two_views.txt of scripts/read_colmap_database.py:52-133 as AddColmapMatchesToReconstructionBuilder reads it
// (src/read_colmap_posegraph.cpp:55-164): three header lines, then per pair
//   "<image1> <image2> f1 f2 num_inliers rot[3] trans[3]" / num_inliers "x y" of image 1 / num_inliers "x y" of image 2.
// View ids follow first appearance (the builder's AddImage order); a pair listed larger-id-first is swapped to
// smaller->larger like GSfMReconstructionBuilder::AddMatchToViewGraph does (SwapCameras, twoview_info.cc:44-62).
// The principal point is half the image size (:77-85); sizes are read from the JPEG/PNG headers of `image_paths`.
// Deviation: the reference pushes the correspondences through theia's TrackBuilder and later recovers an edge's matches
// from the common tracks; here an edge keeps exactly the inlier correspondences listed for it.
struct ColmapPoseGraph {
  std::vector<std::string> view_names;  // index = view id
  std::unordered_map<theia::ViewId, Eigen::Vector2d> principal_point;
  theia::ViewGraph view_graph;
  EdgeMatches matches;
};
bool ReadColmapTwoViews(const std::string& two_views_path, const std::vector<std::string>& image_paths, ColmapPoseGraph* out, std::string* error);
bool ReadImageSize(const std::string& path, int* width, int* height);  // JPEG (SOFn) and PNG (IHDR) headers
std::vector<std::string> ExpandWildcard(const std::string& pattern);

struct CalcCovarianceStats {
  size_t num_edges = 0, num_matches = 0, num_written = 0, num_skipped = 0, num_singular = 0;
  double kernel_ms = 0.0;
};
// bind_src/GlobalSfMpy.cpp:623-628 + store_covariance_rot (src/uncertainty.cpp:164-198): read the dataset, estimate the
// rotation covariance of every edge on the device (one wavefront per edge, gsfm_cov_estimate) and write
// covariance_rot.txt with the refined relative rotation beside it.  Edges the reference skips (zero translation, no
// common track, singular information matrix) are not written.
bool CalcCovariance(const std::string& dataset_directory, CovarianceMap* covariances_or_null, CalcCovarianceStats* stats,
                    std::string* error);
// store_covariance_rot (src/uncertainty.cpp:164-198) on already-flattened matches: the edges of `view_graph` that have
// matches are estimated in one device launch and written to <dir>/covariance_rot.txt.
bool StoreCovarianceRot(const std::string& dataset_directory, const EdgeMatches& matches, const theia::ViewGraph& view_graph,
                        CovarianceMap* covariances_or_null, CalcCovarianceStats* stats, std::string* error);

// residuals_of_relative_rot (src/compare_reconstructions.cpp:617-647): for every edge that has a covariance, the norm of the whitened
// residual Lt log(R_j R_i^T R_ij^T), Lt from 1e8 * Sigma_e, at the given orientations; edges in ViewIdPair order (the reference walks its
// unordered_map).  Edges whose views lack an orientation are skipped.  One device sweep (gsfm_rot_edge_sq_norms); throws without a device.
void ResidualsOfRelativeRotations(const theia::ViewGraph& view_graph, const std::unordered_map<theia::ViewId, Eigen::Vector3d>& orientations,
                                  const CovarianceMap& covariances, std::vector<double>* residuals);
}  // namespace gsfm
