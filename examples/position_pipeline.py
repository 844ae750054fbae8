#!/usr/bin/env python3
"""The reference's scripts/sfm_pipeline.py 1DSfM branch through the full bundle adjustment: rotations, FilterRotations(), OptimizePairwiseTranslations() (every
pair's position_2 refined with the estimated rotations), FilterRelativeTranslation() (the 1DSfM filter), then camera positions
(EstimatePosition(HuberLoss(0.1), PositionErrorType.BASELINE) there; NonlinearPositionEstimator.EstimatePositions here), then
EstimateStructure(refine=True) (every track triangulated, refined per track when the flags say bundle_adjust_tracks, and gated),
SetUnderconstrainedAsUnestimated, BundleAdjustCameraPositionsAndPoints() (camera positions and points adjusted together, orientations and
intrinsics held) and BundleAdjustment() (orientations, positions and points together, intrinsics held: the solve of the script's
BundleAdjustmentAndRemoveOutlierPoints, without its outlier rule), and the PLY with the estimated tracks' points and the estimated camera positions.
usage: position_pipeline.py <dataset_dir with EGs.txt, cc.txt> [flags.yaml]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "globalsfmpy_amd"))  # like sys.path.append('../build')
sys.path.insert(0, os.path.dirname(HERE))

import GlobalSfMpy as sfm  # noqa: E402
from globalsfmpy_amd.loss_functions import HuberLoss  # noqa: E402


SUMMARIES = {}   # of the two bundle adjustments of the last run_pipeline


def run_pipeline(dataset_dir, flagfile=None):
    """(reconstruction, position estimator, reconstruction estimator)"""
    opts = sfm.ReconstructionBuilderOptions()
    if flagfile:
        sfm.load_1DSFM_config(flagfile, opts)
    scene, graph, edge_cov = sfm.Reconstruction(), sfm.ViewGraph(), sfm.MapEdgesCovariance()
    sfm.Read1DSFM(dataset_dir, scene, graph, edge_cov)
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
    solver.EstimateStructure(refine=True)        # a dataset without tracks.txt has nothing to triangulate
    sfm.SetUnderconstrainedAsUnestimated(scene)
    assert solver.BundleAdjustCameraPositionsAndPoints(), solver.LastBundleAdjustmentSummary()
    SUMMARIES["positions and points"] = solver.LastBundleAdjustmentSummary()
    assert solver.BundleAdjustment(), solver.LastBundleAdjustmentSummary()   # orientations, positions and points (intrinsics held)
    SUMMARIES["orientations, positions and points"] = solver.LastBundleAdjustmentSummary()
    return scene, estimator, solver


def position_pipeline(dataset_dir, flagfile=None):
    return run_pipeline(dataset_dir, flagfile)[:2]


if __name__ == "__main__":
    dataset = sys.argv[1]
    scene, estimator, solver = run_pipeline(dataset, sys.argv[2] if len(sys.argv) > 2 else None)
    print("estimated %d positions (view %d held at the origin); solver summary: %s"
          % (len(scene.EstimatedPositions()), estimator.FixedView(), estimator.LastSummary()))
    print("estimated %d of %d tracks" % (scene.NumEstimatedTracks(), scene.NumTracks()))
    for what, summary in SUMMARIES.items():
        print("bundle adjustment of %s: %s" % (what, summary))
    sfm.WritePlyFile(os.path.join(dataset, "positions_out.ply"), scene, 2)
