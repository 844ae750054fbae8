/* gsfm_tracks.h -- C ABI of track triangulation on the GPU (libgsfm_rot.so).
 *
 * Restates Theia's TrackEstimator::EstimateTrack (sfm/estimate_track.cc) with bundle_adjustment = false, the step behind the reference
 * pipeline's reconstruction_estimator.EstimateStructure(): gather a track's observations in estimated views, require a sufficient
 * triangulation angle, triangulate by the midpoint method (triangulation/triangulation.cc: TriangulateMidpoint,
 * SufficientTriangulationAngle), and gate the point on its reprojection error.  The per-track refinement (BundleAdjustTrack) is NOT part
 * of this entry.  Flat arrays in, flat arrays out; every track is an independent small problem in fp64.
 *
 * Cameras (n_cams): rot_aa (n_cams x 3 angle-axis, world -> camera, R = Ceres' AngleAxisToRotationMatrix), cam_pos (n_cams x 3, the
 * camera centre in the world), intrinsics (n_cams x 3: f u v, the pinhole model of gsfm_cov_estimate and of the translation refinement),
 * cam_estimated (n_cams bytes, non-zero = estimated; NULL = every camera is estimated).
 * Tracks (n_tracks): CSR track_ptr[n_tracks + 1] (track_ptr[0] = 0, non-decreasing), obs_cam[n_obs] (camera index of an observation),
 * obs_xy[n_obs x 2] (pixels), n_obs = track_ptr[n_tracks].
 *
 * Per track, over its observations whose camera is estimated, in the order given (n of them; the others are skipped everywhere):
 *   1. ray        r = R^T ((x - u) / f, (y - v) / f, 1),  d = r / |r|,  origin o = cam_pos.
 *   2. n < 2      status 1.
 *   3. angle      c = cos(min_triangulation_angle_degrees pi / 180), computed once on the host in fp64.  The track passes when some pair
 *                 i < j has d_i . d_j < c; otherwise status 2.  A NaN compares false.
 *   4. midpoint   M = sum (I - d d^T),  q = sum (I - d d^T) o = sum (o - d (d . o));  M X = q by a 3 x 3 Cholesky M = L L^T (pivots
 *                 M00, M11 - L10^2, M22 - L20^2 - L21^2; forward then backward substitution).  A pivot that is not positive or not
 *                 finite gives status 3.  Theia solves the 4 x 4 homogeneous system A X~ = b; its last row and column are
 *                 (0, 0, 0, n | n), so the homogeneous coordinate is exactly 1 and the 3 x 3 system above is the same point.  (With
 *                 finite input the angle test rejects every track whose M is singular, so status 3 is there for completeness.)
 *   5. gate       per observation p = R (X - o).  Any p_z < 0: status 4.  Else with the reprojection (f p_x / p_z + u, f p_y / p_z + v)
 *                 the track is accepted, status 0, when the mean over the n observations of the squared pixel error is
 *                 < max_reprojection_error_pixels^2; anything else is status 5 (a NaN mean and p_z = 0 included).
 *                 Theia's Camera::ProjectPoint returns the depth p_z / X~_3 = p_z and the track is rejected on a return value < 0: the
 *                 same rule; p_z = 0 passes Theia's depth test too and fails on the infinite or NaN mean, as here.  Theia stops at the
 *                 first observation behind its camera; the result does not depend on which one that is.  Departure that decides nothing
 *                 at the tolerances of interest: Theia rotates with AngleAxisRotatePoint, here p is formed with the matrix R.
 * status_out per track:  0 estimated;  1 fewer than 2 observations in estimated views;  2 insufficient triangulation angle;
 *   3 the Cholesky failed;  4 the point lies behind a camera;  5 reprojection error too high.
 *   Theia's log reports 1 and 2 together as "bad triangulation angles", 3 as failed triangulations, 4 and 5 together as
 *   "too high reprojection errors".
 * Outputs: point_out (n_tracks x 3: X for the statuses 0, 4 and 5, zero otherwise), status_out (n_tracks); optional (NULL: not returned)
 * n_views_out (n_tracks: the count n), mean_sq_err_out (n_tracks: the mean of step 5 over all n observations for the statuses 0, 4 and 5,
 * zero otherwise), counts_out[6] (tracks per status), kernel_ms (device time of the kernels).
 *
 * Order of the sums (part of the definition: it decides the rounding).  A track of `len` observations (its CSR length, estimated or not)
 * is worked by a group of G lanes:
 *        len <= 8: G = 4;      9 <= len <= 64: G = 16;      len >= 65: G = 64.
 * Lane l of the group adds the terms of the observations at places l, l + G, l + 2G, ... of the track, in that order, starting from 0
 * (the nine sums of M and q in step 4, the squared errors in step 5); the G partial sums are then combined by an xor butterfly with the
 * offsets G/2, G/4, ..., 1 (v += v of lane l xor offset).  The order depends on the track's own length and data alone: two calls return
 * the same bytes, and permuting the tracks permutes the outputs bit for bit.  The tracks run in the order gsfm_tracks_launch_order gives;
 * outputs are written at the caller's index.
 *
 * Device memory 20 B per observation (+ 24 B per observation when a track of 65 or more observations exists) + O(n_tracks + n_cams).
 * Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: a NULL required pointer, track_ptr[0] != 0, a track_ptr
 * that decreases, a camera index >= n_cams, an angle or an error bound that is negative or not finite); without a device
 * GSFM_ERR_NO_DEVICE: there is no host fallback.  No tracks: GSFM_OK. */
#ifndef GSFM_TRACKS_H_
#define GSFM_TRACKS_H_

#include <stdint.h>
#include "gsfm_rot.h"

#ifdef __cplusplus
extern "C" {
#endif

gsfm_status gsfm_tracks_triangulate(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                    const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                    const double* obs_xy, double min_triangulation_angle_degrees, double max_reprojection_error_pixels,
                                    double* point_out, int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out,
                                    uint64_t* counts_out, double* kernel_ms);

/* The launch order of gsfm_tracks_triangulate, host code only (no device is touched): order_out[n_tracks] lists the tracks of lane class
 * G = 4, then 16, then 64, inside a class by descending length and equal lengths by ascending index; class_begin_out[4] holds the three
 * slices' bounds in order_out.  GSFM_ERR_INVALID_ARG for a NULL pointer (n_tracks > 0), a decreasing track_ptr or 2^31 or more tracks. */
gsfm_status gsfm_tracks_launch_order(uint64_t n_tracks, const uint64_t* track_ptr, uint32_t* order_out, uint64_t* class_begin_out);

/* ---- Triangulation WITH the per-track refinement: gsfm_tracks_triangulate_refine ----
 *
 * Restates EstimateTrack with bundle_adjustment = true: between the midpoint (step 4) and the gate (step 5) Theia runs BundleAdjustTrack
 * (sfm/bundle_adjustment/bundle_adjust_track.cc), a Levenberg-Marquardt on the point alone with every camera held constant, and gates
 * the refined point.  The arguments of gsfm_tracks_triangulate, the options below and a loss; the steps 1 to 4 are those above, to the
 * bit, and so is step 5 on the point it is given.
 *
 * The loss is a descriptor of gsfm_rot.h, passed as gsfm_pos_set_loss takes one: loss_program / n_loss_nodes, n_loss_nodes = 0 being
 * Ceres' NULL loss.  Accepted: ONE leaf of the kinds GSFM_LOSS_TRIVIAL (Theia's TRIVIAL), GSFM_LOSS_HUBER (p0 = a; the reference's YAML:
 * HUBER, width 10), GSFM_LOSS_SOFT_L1, GSFM_LOSS_TUKEY, GSFM_LOSS_GEMAN_MCCLURE; a width (p0) that is not positive, a parameter that is
 * not finite, every other leaf (MAGSAC among them) and every program of more than one node are GSFM_ERR_INVALID_ARG.
 *
 * Per track that has status 0 after step 4, with the midpoint X_0:
 *   parameters  the three inhomogeneous coordinates X.  DEPARTURE: Theia optimises the homogeneous 4-vector without a local
 *               parameterisation; its scale direction is a gauge of the cost, so the minimiser is the same projective point.
 *   residual    per observation in an estimated view, in the track's order: p = R (X - o), r = (f p_x / p_z + u - x, f p_y / p_z + v - y),
 *               s = |r|^2; cost = 1/2 sum rho(s).  Jacobian J = (f / p_z) [[1, 0, -p_x / p_z], [0, 1, -p_y / p_z]] R.  Robustified by
 *               Ceres' Corrector (corrector.cc): with (rho, rho', rho'')(s), J <- sqrt(rho') (J - alpha / s r r^T J), r <- sqrt(rho') /
 *               (1 - alpha) r, alpha = 1 - sqrt(1 + 2 s rho'' / rho') where s > 0 and rho'' > 0, else alpha = 0.
 *   a pass      at a point: the ten sums S = J^T J (xx xy xz yy yz zz), g = J^T r (x y z) and the cost, of the corrected J and r.
 *   start       pass at X_0.  Jacobi scaling c_k = 1 / (1 + sqrt(S_kk)), kept for the whole solve.  radius = initial_trust_region_radius,
 *               decrease factor 2, iteration count 0.  A cost that is not finite: FAILURE.  max |g_k| <= gradient_tolerance: GRADIENT_
 *               TOLERANCE.  max_num_iterations = 0: NO_CONVERGENCE.  (In this order; the termination codes are gsfm_rot_termination's.)
 *   iteration   count += 1.  In the scaled space A = diag(c) S diag(c), b = diag(c) g, D2_k = min(max(A_kk, 1e-6), 1e32):
 *               (A + diag(D2) / radius) e = -b by the 3 x 3 Cholesky of step 4 (pivots as there), d = diag(c) e.
 *               model change m = -d . g - 1/2 d^T S d  (= -(J d)^T (r + J d / 2)).  A pivot that is not positive or not finite, or an m
 *               that is not finite or not > 0, or a trial cost (pass at X + d) that is not finite, is an INVALID step: the fifth in
 *               a row is FAILURE, otherwise radius /= decrease factor, decrease factor *= 2.
 *               Valid step: |d| <= parameter_tolerance (|X| + parameter_tolerance): PARAMETER_TOLERANCE.  Else |cost - trial cost| <=
 *               function_tolerance cost: FUNCTION_TOLERANCE.  (A terminating step is not applied.)  Else q = (cost - trial cost) / m:
 *               q > min_relative_decrease accepts -- X += d, the trial's pass is the iterate's, radius = min(max_trust_region_radius,
 *               radius / max(1/3, 1 - (2 q - 1)^3)), decrease factor = 2; otherwise radius /= decrease factor, decrease factor *= 2.
 *               Then: count >= max_num_iterations: NO_CONVERGENCE; else after an accepted step max |g_k| <= gradient_tolerance:
 *               GRADIENT_TOLERANCE; else radius <= min_trust_region_radius: FAILURE.
 *               These are the rules of Ceres 1.14's TrustRegionMinimizer with the LEVENBERG_MARQUARDT strategy, as gsfm_rot_solve and
 *               gsfm_pos_solve restate them.  DEPARTURES: Theia's solve is DENSE_QR on the 2n x 4 Jacobian where this solves the
 *               normal equations; Theia rotates with AngleAxisRotatePoint where p is formed with the matrix R, as in step 5.
 *   status      FAILURE is the new status 6, "refinement failed" (Theia: !summary.success; the track is dropped and counted nowhere in its
 *               log): point and mean are zero.  Every other termination goes on to step 5 with the refined X; 0, 4 and 5 mean what they
 *               mean above.
 * options->refine = 0 skips all of this: the call is gsfm_tracks_triangulate's, with its kernels and its bytes.  options = NULL: the
 * defaults, gsfm_tracks_refine_default_options (refine = 1; the tolerances of Theia's BundleAdjustmentOptions and of Ceres).
 * max_num_iterations is clamped to 0 .. 1000.  Tolerances that are negative or not finite, radii that are not positive and finite (the
 * minimum may be 0): GSFM_ERR_INVALID_ARG.
 *
 * Order of the sums (part of the definition).  The ten sums of a pass are taken exactly like those of steps 4 and 5: lane l of the
 * track's group of G lanes adds the terms of the observations at places l, l + G, ... in that order, starting from 0 (the cost's term is
 * rho(s) / 2), then the xor butterfly.  Every scalar decision is taken on the butterfly's sums, which are the same in all lanes: a track's
 * iterates depend on its own length and data alone, whatever shares its wavefront -- two calls return the same bytes, permuting the tracks
 * permutes the outputs bit for bit, and a track run alone returns what it returns inside a batch.
 *
 * Outputs: those of gsfm_tracks_triangulate, and optional (NULL: not returned) per track iterations_out (the count), initial_cost_out (the
 * cost at X_0), final_cost_out (the cost at the X that went to step 5), termination_out (gsfm_rot_termination) -- 0, 0, 0 and -1 for a
 * track that was not refined (status 1, 2, 3, or refine = 0); counts_out[7] (tracks per status).  Device memory: 24 B per track more. */
typedef struct {
  int32_t refine;                      /* 0: no refinement */
  int32_t max_num_iterations;          /* 100 */
  double function_tolerance;           /* 1e-6 */
  double gradient_tolerance;           /* 1e-10 */
  double parameter_tolerance;          /* 1e-8 */
  double min_relative_decrease;        /* 1e-3 */
  double initial_trust_region_radius;  /* 1e4 */
  double max_trust_region_radius;      /* 1e12 (Theia's BundleAdjustmentOptions) */
  double min_trust_region_radius;      /* 1e-32 */
} gsfm_tracks_refine_options;

void gsfm_tracks_refine_default_options(gsfm_tracks_refine_options* options);

gsfm_status gsfm_tracks_triangulate_refine(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                           const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                           const double* obs_xy, double min_triangulation_angle_degrees, double max_reprojection_error_pixels,
                                           const gsfm_tracks_refine_options* options, const gsfm_loss_node* loss_program, int32_t n_loss_nodes,
                                           double* point_out, int32_t* status_out, int32_t* n_views_out, double* mean_sq_err_out,
                                           int32_t* iterations_out, double* initial_cost_out, double* final_cost_out, int32_t* termination_out,
                                           uint64_t* counts_out, double* kernel_ms);

/* ---- The outlier rule after a bundle adjustment: gsfm_tracks_outlier_tracks ----
 *
 * Restates Theia's SetOutlierTracksToUnestimated (sfm/set_outlier_tracks_to_unestimated.cc), the second half of the reference pipeline's
 * BundleAdjustmentAndRemoveOutlierPoints(): every estimated track is tested on the reprojection error of its point and on the angle under
 * which its estimated views see that point.  The cameras and tracks of gsfm_tracks_triangulate, with the same meaning and the same checks;
 * points (n_tracks x 3, the tracks' points in the world) and point_estimated (n_tracks bytes, non-zero = estimated; NULL = every track is
 * estimated).  Nothing is written to the inputs: the caller clears the flags of the statuses 2 to 4.
 *
 * Per track that is estimated on input, over its observations whose camera is estimated, in the order given (n of them; the others are
 * skipped everywhere), with the track's point X:
 *   1. gate quantities   step 5 of gsfm_tracks_triangulate on X, its text unchanged: p = R (X - o) per observation, behind = some p_z < 0,
 *                        mean = sum |(f p_x / p_z + u, f p_y / p_z + v) - (x, y)|^2 / n, the sum in that entry's order (below).  Given the
 *                        point gsfm_tracks_triangulate returned for a track, mean_sq_err_out is that call's mean_sq_err_out bit for bit.
 *   2. ray               d = (X - o) / |X - o|, |v| = sqrt(v_x^2 + v_y^2 + v_z^2), in the world frame: Theia's Point().hnormalized() -
 *                        GetPosition(), normalised.  It comes from the point, not from the pixel.  A point at a camera centre gives a NaN
 *                        ray, which passes no comparison.
 *   3. status, decided in this order:
 *        2  behind: some p_z < 0.  Theia counts this as a bad reprojection; it stops at the first such view, and the result does not depend
 *           on which one that is.
 *        3  mean > max_reprojection_error_pixels^2.  Strict, as in Theia: a NaN mean (p_z = 0 with p_x = 0, or n = 0) is NOT removed here and
 *           goes on to the angle test; +inf is removed.
 *        4  no pair i < j with d_i . d_j < c, c = cos(min_triangulation_angle_degrees pi / 180) computed once on the host in fp64 (step 3 of
 *           gsfm_tracks_triangulate on these rays).  n < 2 lands here, n = 0 included, as Theia's empty loop does.
 *        0  kept.
 *   A track that is not estimated on input is status 1: it is not examined and its optional outputs are 0.
 *   Departure that decides nothing at the tolerances of interest: p is formed with the matrix R, as in gsfm_tracks_triangulate.
 * Outputs: status_out (n_tracks, required); optional (NULL: not returned) n_views_out (n_tracks: the count n), mean_sq_err_out (n_tracks: the
 * mean of step 1, whatever the status 0, 2, 3 or 4; NaN where n = 0), counts_out[5] (tracks per status; Theia's return value is
 * counts[2] + counts[3] + counts[4], its log reports 2 and 3 together as bad reprojection errors and 4 alone as insufficient viewing angles),
 * kernel_ms (device time of the kernels).
 *
 * Order of the sums: that of gsfm_tracks_triangulate.  The lane class is a function of the track's CSR length (len <= 8: G = 4;
 * 9 <= len <= 64: G = 16; len >= 65: G = 64), lane l adds the squared errors of the observations at places l, l + G, ... in that order
 * starting from 0, then the xor butterfly.  A track's result depends on its own length and data alone: two calls return the same bytes,
 * permuting the tracks permutes the outputs bit for bit, and another track's point_estimated changes nothing for this one.  The estimated
 * tracks run in the order gsfm_tracks_launch_order gives (the others are left out of it and never reach the device).
 *
 * Device memory: that of gsfm_tracks_triangulate, 20 B per observation (+ 24 B per observation when an estimated track of 65 or more
 * observations exists) + 52 B per track + O(n_cams); the points take the place of that entry's point_out and point_estimated stays on the host.
 * GSFM_ERR_INVALID_ARG before any device call by the rules of gsfm_tracks_triangulate, and for NULL points, NULL status_out, a bound or an
 * angle that is negative or not finite.  No tracks, or none estimated: GSFM_OK with kernel_ms = 0 and no device call.  Otherwise without a
 * device GSFM_ERR_NO_DEVICE: there is no host fallback. */
gsfm_status gsfm_tracks_outlier_tracks(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                       const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                       const double* obs_xy, const double* points, const uint8_t* point_estimated,
                                       double max_reprojection_error_pixels, double min_triangulation_angle_degrees, int32_t* status_out,
                                       int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms);

/* ---- Tracks from two-view matches: gsfm_tracks_build ----
 *
 * Restates Theia's TrackBuilder (sfm/track_builder.cc over math/graph/connected_components.h), which the reference's COLMAP branch runs when
 * the reconstruction has no tracks: every inlier match of every view pair is one AddFeatureCorrespondence, BuildTracks turns the connected
 * components into tracks.
 *
 * Input: n_edges view pairs (edge_i[e], edge_j[e], both < n_views and different), the CSR match_ptr[n_edges + 1] (match_ptr[0] = 0,
 * non-decreasing), matches (n_matches x 4: x1 y1 of view edge_i, x2 y2 of view edge_j, pixels), n_matches = match_ptr[n_edges], in the
 * caller's order: match m stands for the m-th call of AddFeatureCorrespondence.
 *
 *   endpoints   endpoint 2m is the first feature of match m (view edge_i, x1 y1), endpoint 2m + 1 its second (view edge_j, x2 y2).
 *   features    two endpoints are the same feature when they have the same view and equal coordinates, compared as doubles: -0.0 equals 0.0.
 *               A coordinate that is not finite is GSFM_ERR_INVALID_ARG.  A feature's representative is its smallest endpoint index; the
 *               feature's id is the rank of its representative among all representatives: Theia's FindOrInsert numbering for this order
 *               of calls.  The feature's pixel is its representative's, bit for bit (so of -0.0 and 0.0 the first one met).
 *   components  each match joins its two features.  The plain components are those of that graph; a component's label is its smallest
 *               feature id.  Theia refuses a union that would make a component larger than max_track_length (connected_components.h:87-108:
 *               nothing happens when both features share a root or when the two sizes add up to more than the maximum), in call order.
 *               A plain component of at most max_track_length features never met a refusal and is final.  The matches of every larger
 *               plain component are replayed in the caller's order under that rule -- on the host, sequentially: the path is rare with
 *               the reference's max_track_length of 1000 -- and the pieces they end in take its place, each labelled by its smallest
 *               feature id.  That gives Theia's components for the same order of calls.
 *   tracks      walking the final components by ascending label:
 *                 fewer than min_track_length features: dropped, counted `small` (before any duplicate removal, as in Theia);
 *                 its features in ascending feature id; a feature whose view already occurs earlier in the track is dropped, counted
 *                 `inconsistent`.  DEPARTURE: Theia keeps whichever feature of a view its unordered_set yields first;
 *                 fewer than two observations left: the track is dropped, counted `degenerate` (Theia would abort in AddTrack).  Since a
 *                 match joins two views this needs a component of one feature, that is min_track_length <= 1 and a refused union;
 *                 otherwise a track: its observations are (view, pixel) of the kept features in that order.
 * Outputs (the caller provides the capacity: n_matches + 1 offsets, 2 n_matches observations): track_ptr_out (CSR, track_ptr_out[0] = 0),
 * obs_view_out, obs_xy_out (x y per observation), *n_tracks, *n_obs; optional (NULL: not returned) counts_out[7] = features, final
 * components, small, inconsistent, degenerate, replayed (the plain components larger than max_track_length), tracks; kernel_ms (device time
 * of the kernels, the waits of the host's looks at the component rounds included).
 * The output is a pure function of the input arrays: two calls return the same bytes, whatever lane wins a hash slot or an atomic.
 *
 * Options (NULL: the defaults): min_track_length 2, max_track_length 1000 (both Theia's and the reference's flag files'), both >= 1;
 * hash_capacity_log2: the feature table has 2^hash_capacity_log2 slots, 0 = automatic (the smallest power of two >= 4 n_matches, at least
 * 2^10).  It exists so that a test can force long probe chains: a capacity below the number of endpoints (2 n_matches), or above 2^31, is
 * GSFM_ERR_INVALID_ARG, not a hang.
 *
 * Device memory about 300 B per match.  Arguments are checked on the host before any device call (GSFM_ERR_INVALID_ARG: a NULL required
 * pointer, match_ptr[0] != 0, a match_ptr that decreases, a view index >= n_views, an edge from a view to itself, more than 2^29 matches,
 * a coordinate that is not finite, an option out of range); no matches: GSFM_OK with no track and no device call; otherwise without a
 * device GSFM_ERR_NO_DEVICE: there is no host fallback.
 *
 * gsfm_tracks_build_sequential is the same definition as plain sequential host code (hash map, union-find with the refusal rule over all
 * matches, no device is touched): the replay above is its union rule; it is the host baseline of tools/time_track_build.py and a test
 * reference.  hash_capacity_log2 is checked and otherwise ignored; kernel_ms is 0. */
typedef struct {
  int32_t min_track_length;    /* 2 */
  int32_t max_track_length;    /* 1000 */
  int32_t hash_capacity_log2;  /* 0: automatic */
} gsfm_tracks_build_options;

void gsfm_tracks_build_default_options(gsfm_tracks_build_options* options);

gsfm_status gsfm_tracks_build(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j, const uint64_t* match_ptr,
                              const double* matches, const gsfm_tracks_build_options* options, uint64_t* track_ptr_out, uint32_t* obs_view_out,
                              double* obs_xy_out, uint64_t* n_tracks, uint64_t* n_obs, uint64_t* counts_out, double* kernel_ms);
gsfm_status gsfm_tracks_build_sequential(uint32_t n_views, uint64_t n_edges, const uint32_t* edge_i, const uint32_t* edge_j,
                                         const uint64_t* match_ptr, const double* matches, const gsfm_tracks_build_options* options,
                                         uint64_t* track_ptr_out, uint32_t* obs_view_out, double* obs_xy_out, uint64_t* n_tracks, uint64_t* n_obs,
                                         uint64_t* counts_out, double* kernel_ms);

/* ---- The tracks a bundle adjustment is given: gsfm_tracks_select_good ----
 *
 * Restates Theia's SelectGoodTracksForBundleAdjustment (sfm/select_good_tracks_for_bundle_adjustment.cc), which the reference pipeline's
 * BundleAdjustment() and BundleAdjustCameraPositionsAndPoints() call under subsample_tracks_for_bundle_adjustment: per view and cell of an
 * image grid the best track, then every view topped up to a minimum number of tracks.  The bundle solvers take the result as point_estimated.
 *
 * Input: the cameras and tracks of gsfm_tracks_outlier_tracks, with the same meaning and the same host checks (rot_aa, cam_pos, intrinsics,
 * cam_estimated, track_ptr, obs_cam, obs_xy, points, point_estimated), and long_track_length_threshold L >= 1, image_grid_cell_size_pixels
 * S >= 1, min_num_optimized_tracks_per_view K >= 0 (Theia's header defaults: 10, 100, 200; the reference's flag files say 100 for K).
 * An ITEM is one observation of an estimated track in an estimated camera.  A track that lists a camera twice cannot exist in Theia (a View
 * holds one feature per track); here each such observation is an item of its own, in the device code and the sequential code alike.
 *
 *   1. statistics  per estimated track, over its observations in estimated cameras in the order given: n their count; mean = step 1 of
 *                  gsfm_tracks_outlier_tracks, its text and its summation order unchanged: it equals that entry's mean_sq_err_out bit for
 *                  bit.  There is no depth test (Theia's ComputeSqReprojectionError has none).  A track with n = 0 has no item and can never
 *                  be selected.  The track's key is (min(n, L), mean), compared lexicographically, the mean by its bit pattern as an unsigned
 *                  64-bit integer after every NaN has been replaced by 0x7ff8000000000000: means are >= +0, so bit order is numeric order,
 *                  +inf comes after every finite value and NaN after +inf.  A SMALLER key is better -- the shorter truncated length first:
 *                  Theia's CompareGridCellElements (element1.second < element2.second over TrackStatistics = pair<length, error>), literally.
 *   2. grid cells  with inv = 1.0 / (double)S an item lies in the cell (camera, (int32)trunc(x inv), (int32)trunc(y inv)): one multiplication
 *                  and a truncation toward zero, Eigen's cast<int>().  A coordinate that is not finite or has |x inv| >= 2^31 is
 *                  GSFM_ERR_INVALID_ARG before any device call.  Per non-empty cell the item with the smallest key is chosen, equal keys
 *                  going to the smallest track index; its track is selected, selected_out = 1.
 *                  DEPARTURE: of equal keys Theia keeps the first in the hash-set order of the view's tracks.
 *                  DEPARTURE: Theia's inv_grid_cell_size is a function-local static, so the first call's cell size holds for the whole
 *                  process; here every call uses its own S.
 *   3. top-up      the cameras in ascending index (DEPARTURE: Theia walks an unordered_set of views and its result depends on that order).
 *                  For camera v: est = its number of items, opt = the number of those whose track is selected at that moment, the tracks
 *                  earlier cameras' top-ups added included.  K = 0, opt >= K or opt = est: nothing happens.  Otherwise m = min(K - opt,
 *                  est - opt) and the first m items of v whose track is not selected as v's turn begins, walked by ascending (track index,
 *                  place in the track), are taken: their tracks are selected, selected_out = 2.
 *                  This is the literal restatement: Theia's std::partial_sort over pair<TrackId, TrackStatistics> has no comparator, so it
 *                  orders by track id first and the statistics never decide.  The evidently intended ranking by statistics is not built.
 * Outputs: selected_out (n_tracks bytes, required): 0, 1 (by a cell) or 2 (by the top-up); 0 for every track not estimated on input.
 * Optional (NULL: not returned): n_views_out, mean_sq_err_out (per track: n and mean of step 1, NaN where n = 0; both 0 for a track that is not
 * estimated), counts_out[6] = tracks with n >= 1, non-empty cells, tracks selected by a cell, cameras that needed a top-up, tracks selected by
 * the top-up, tracks selected in all; kernel_ms (device time of the kernels); top_up_out[2] = the number of items the host downloaded for
 * step 3, the milliseconds its replay took.
 * The output is a pure function of the input arrays: two calls return the same bytes, whatever lane wins a slot or an atomic.
 *
 * On the device: the statistics in the lane classes and the launch order of gsfm_tracks_outlier_tracks over the estimated tracks; step 2 in an
 * open-addressing table of cells over all items (slots claimed by compare-and-swap, then three sweeps of integer atomic minima: truncated
 * length, canonical mean bits among the items of that length, track index among those of both); est and opt per camera by integer atomics.
 * A camera is deficient when K > 0, opt < K and opt < est after step 2; counts only grow during step 3, so no other camera can need a top-up.
 * The items of the deficient cameras are compacted to a list the host downloads, sorts by (camera, track, place) and walks as step 3 says --
 * step 3 is sequential across cameras by definition; the precedent is the max_track_length replay of gsfm_tracks_build.
 * hash_capacity_log2: the cell table has 2^hash_capacity_log2 slots, 0 = automatic (the smallest power of two >= 2 x items, at least 2^10).
 * It exists so that a test can force long probe chains: a capacity below the number of items, or above 2^31, is GSFM_ERR_INVALID_ARG, not a hang.
 *
 * Device memory 40 B per observation + 20 B per table slot + 53 B per track + O(n_cams).  GSFM_ERR_INVALID_ARG before any device call by the
 * rules of gsfm_tracks_triangulate, and for NULL points, NULL selected_out, L < 1, S < 1, K < 0, 2^31 or more observations, a coordinate off
 * the grid, a hash_capacity_log2 out of range.  No tracks, or none estimated: GSFM_OK with no device call.  Otherwise without a device
 * GSFM_ERR_NO_DEVICE: there is no host fallback.
 *
 * gsfm_tracks_select_good_from_statistics runs steps 2 and 3 as plain sequential host code (a hash map of cells; no device is touched) on
 * statistics it is given: n_views and mean_sq_err per track (read for the estimated tracks; a negative n_views there is
 * GSFM_ERR_INVALID_ARG).  The items are decided by cam_estimated and point_estimated as above.  It writes selected_out and counts_out; it is
 * the host baseline of tools/time_track_selection.py and a test reference. */
gsfm_status gsfm_tracks_select_good(uint32_t n_cams, const double* rot_aa, const double* cam_pos, const double* intrinsics,
                                    const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr, const uint32_t* obs_cam,
                                    const double* obs_xy, const double* points, const uint8_t* point_estimated,
                                    int32_t long_track_length_threshold, int32_t image_grid_cell_size_pixels,
                                    int32_t min_num_optimized_tracks_per_view, int32_t hash_capacity_log2, uint8_t* selected_out,
                                    int32_t* n_views_out, double* mean_sq_err_out, uint64_t* counts_out, double* kernel_ms, double* top_up_out);
gsfm_status gsfm_tracks_select_good_from_statistics(uint32_t n_cams, const uint8_t* cam_estimated, uint64_t n_tracks, const uint64_t* track_ptr,
                                                    const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                                    const int32_t* n_views, const double* mean_sq_err, int32_t long_track_length_threshold,
                                                    int32_t image_grid_cell_size_pixels, int32_t min_num_optimized_tracks_per_view,
                                                    uint8_t* selected_out, uint64_t* counts_out);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_TRACKS_H_ */
