#!/usr/bin/env python3
"""The reference's scripts/sfm_pipeline.py 1DSfM branch to its end: the calls of position_pipeline.py up to
SetReconstructionFromEstimatedPoses (rotations, FilterRotations(), OptimizePairwiseTranslations(), FilterRelativeTranslation(), camera
positions), then the script's structure loop, 1 + num_retriangulation_iterations times:
    EstimateStructure(refine=True, only_unestimated=True)    the tracks that are not estimated are triangulated (and refined per track when
                                                             the flags say bundle_adjust_tracks); estimated tracks keep their points
    SetUnderconstrainedAsUnestimated
    BundleAdjustCameraPositionsAndPoints()                   first pass only, when refine_camera_positions_and_points_after_position_estimation
    BundleAdjustmentAndRemoveOutlierPoints()                 BundleAdjustment(), then SetOutlierTracksToUnestimated(max_reprojection_error_in_pixels,
                                                             min_triangulation_angle_degrees) when the solution is usable
and the PLY with the estimated tracks' points and the estimated camera positions.
With use1DSfM=False the script's COLMAP branch: the view graph and the matches come from two_views.txt (AddColmapMatchesToReconstructionBuilder),
CheckView() builds the tracks from the matches on the device (Theia's TrackBuilder, include/gsfm_tracks.h), and the same calls follow.
usage: reconstruction_pipeline.py <dataset_dir with EGs.txt, cc.txt, tracks.txt, coords.txt, list.txt> [flags.yaml]
       reconstruction_pipeline.py --colmap <dataset_dir with two_views.txt and images/> [flags.yaml] [images wildcard]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "globalsfmpy_amd"))  # like sys.path.append('../build')
sys.path.insert(0, os.path.dirname(HERE))

import GlobalSfMpy as sfm  # noqa: E402
from globalsfmpy_amd.loss_functions import HuberLoss  # noqa: E402


def run_pipeline(dataset_dir, flagfile=None, use1DSfM=True, images_wildcard=None):
    """(reconstruction, reconstruction estimator, passes): per pass of the structure loop the structure summary, the estimated-track counts
    around the outlier step, and the summaries of the adjustments"""
    opts = sfm.ReconstructionBuilderOptions()
    if flagfile:
        sfm.load_1DSFM_config(flagfile, opts)
    if use1DSfM:
        scene, graph, edge_cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
        sfm.Read1DSFM(dataset_dir, scene, graph, edge_cov)
    else:   # sfm_pipeline.py:39-52
        builder = sfm.ReconstructionBuilder(opts, sfm.FeaturesAndMatchesDatabase(os.path.join(dataset_dir, "database")))
        sfm.AddColmapMatchesToReconstructionBuilder(os.path.join(dataset_dir, "two_views.txt"),
                                                    images_wildcard or os.path.join(dataset_dir, "images", "*.JPG"), builder)
        builder.CheckView()   # no tracks yet: built from the matches
        graph, scene = builder.get_view_graph(), builder.get_reconstruction()
    solver = sfm.GlobalReconstructionEstimator(opts.reconstruction_estimator_options)
    solver.FilterInitialViewGraphAndCalibrateCameras(graph, scene)
    assert solver.EstimateGlobalRotations(HuberLoss(0.1)), solver.LastError()
    solver.FilterRotations()
    solver.OptimizePairwiseTranslations()
    solver.FilterRelativeTranslation()
    positions = sfm.MapViewIdVector3d()
    estimator = sfm.NonlinearPositionEstimator()
    assert estimator.EstimatePositions(graph.GetAllEdges(), solver.orientations, positions, HuberLoss(0.1),
                                       sfm.PositionErrorType.BASELINE), estimator.LastError()
    sfm.SetReconstructionFromEstimatedPoses(solver.orientations, positions, scene)
    # always triangulate once, then retriangulate and remove outliers as the options say (sfm_pipeline.py:92-107)
    passes = []
    for i in range(1 + solver.options.num_retriangulation_iterations):
        record = {"structure": solver.EstimateStructure(refine=True, only_unestimated=True)}
        record["underconstrained"] = sfm.SetUnderconstrainedAsUnestimated(scene)
        if i == 0 and solver.options.refine_camera_positions_and_points_after_position_estimation:
            solver.BundleAdjustCameraPositionsAndPoints()
            record["positions_and_points"] = solver.LastBundleAdjustmentSummary()
        record["estimated_before_outlier_step"] = scene.NumEstimatedTracks()
        record["bundle_adjustment"] = solver.BundleAdjustmentAndRemoveOutlierPoints()
        record["outliers"] = solver.LastOutlierSummary()
        record["estimated_after_outlier_step"] = scene.NumEstimatedTracks()
        passes.append(record)
    return scene, solver, passes


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--colmap"]
    dataset = argv[0]
    scene, solver, passes = run_pipeline(dataset, argv[1] if len(argv) > 1 else None, use1DSfM="--colmap" not in sys.argv,
                                         images_wildcard=argv[2] if len(argv) > 2 else None)
    if scene.LastTrackBuildSummary():
        print("tracks from matches: %(tracks)d tracks of %(features)d features (%(small)d small, %(inconsistent)d inconsistent features dropped)"
              % scene.LastTrackBuildSummary())
    for i, record in enumerate(passes):
        print("pass %d: triangulated %d of %d unestimated tracks; bundle adjustment %s; %d outlier tracks removed, %d tracks estimated"
              % (i, record["structure"]["num_estimated"], record["structure"]["num_tracks"],
                 "usable" if record["bundle_adjustment"]["success"] else "FAILED", record["bundle_adjustment"]["num_points_removed"],
                 record["estimated_after_outlier_step"]))
    print("estimated %d positions and %d of %d tracks" % (len(scene.EstimatedPositions()), scene.NumEstimatedTracks(), scene.NumTracks()))
    sfm.WritePlyFile(os.path.join(dataset, "reconstruction_out.ply"), scene, 2)
