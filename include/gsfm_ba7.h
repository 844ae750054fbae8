/* gsfm_ba7.h -- C ABI of the full bundle adjustment with free focal lengths on the GPU: camera orientations, camera positions, focal lengths
 * and points (libgsfm_rot.so).
 *
 * Restates the solve of Theia's GlobalReconstructionEstimator::BundleAdjustment() with intrinsics_to_optimize = FOCAL_LENGTH (what the
 * reference's flags.yaml sets; its flags_1dsfm.yaml sets NONE, which is gsfm_ba6.h).  gsfm_ba6.h is the same problem with the focal lengths
 * held; this header follows it and states only what differs.
 *
 * Inputs are those of gsfm_ba6_problem_create, with one more flag array, focal_free.  The principal point u v of a camera is held and comes
 * from columns 1 and 2 of `intrinsics` (n_cams x 3) at create; column 0 is NOT read: the focal length (n_cams, in pixels) is a start value
 * and an unknown, an argument of the solve as rot_aa is in gsfm_ba6.h.
 *
 * Definition.
 *   unknowns   per active camera w_k, o_k and the focal length f_k, per active point X_t.  f_k is optimised directly, as Theia optimises it:
 *              no logarithm or other reparameterisation, no bounds.
 *   residual   unchanged: r = (f p_x / p_z + u - x, f p_y / p_z + v - y).
 *   Jacobian   the pieces of gsfm_ba6.h and J_f = (p_x / p_z, p_y / p_z)^T (2 x 1).  Ceres' Corrector mixes its two entries exactly as it
 *              mixes the rows of the other pieces: J~_f = sqrt(rho') (J_f - alpha / s r r^T J_f).
 *   normal matrix   Jc_e = [J~_rot, -J~_point, J~_f] (2 x 7); B_k = sum Jc^T Jc is 7 x 7, coordinates w, o, f; E_e = Jc^T Jp is 7 x 3; g_k has 7
 *              entries.
 *   LM         the rules of gsfm_ba.h / gsfm_ba6.h over 7 coordinates per camera.  Jacobi scaling and the diagonal clamp act on the focal
 *              coordinate like on any other.  The function, gradient and parameter tolerances take their norms over all active coordinates,
 *              the focal lengths included, as Ceres does; |x| is then DOMINATED BY THE FOCALS (hundreds to thousands of pixels each, against
 *              centres and points of order one to ten), so the parameter tolerance |delta| <= parameter_tolerance (|x| + parameter_tolerance)
 *              is looser in absolute terms than in gsfm_ba6.h on the same scene.  gsfm_ba_options and gsfm_ba_summary are reused;
 *              gsfm_ba7_options_default is gsfm_ba6_options_default (PCG to 1e-14) but for cg_stall_iterations, see below.
 *   linear solve    as gsfm_ba6.h: the points eliminated through the double-double inverse, the reduced camera system (7 x 7 diagonal blocks)
 *              solved matrix-free by PCG; one product is a point pass and a camera pass over the corrected Jacobians, 14 doubles per
 *              observation.  The preconditioner is the 7 x 7 block diagonal of Sc, inverted per camera through its Cholesky factor.
 *   gauge      the seven directions of gsfm_ba6.h with a zero focal component: with a known principal point the focal length is no gauge
 *              freedom.  J V = 0 still holds and the 7 x 7 Gram solve is unchanged.
 *   focal_free optional uint8 per camera at create; NULL means every active camera.  A camera with focal_free = 0 is adjusted as in
 *              gsfm_ba6.h with the focal length passed to the solve held: its focal coordinate is no parameter (it enters no norm, its
 *              gradient entry, its row and column of B_k and its step are exact zeros, the PCG operator is the identity on it), and its
 *              focal length is returned bit for bit.  One focal length per camera: shared calibration groups are not built.
 *
 * Order of the sums: gsfm_ba6.h's.  No atomics: two solves return the same bytes.
 *
 * DEPARTURES from the reference: those of gsfm_ba6.h except (6), and (7) the preconditioner: Ceres' SCHUR_JACOBI would use a 6 x 6 block
 * (the extrinsics) and a 1 x 1 block (the intrinsics are a parameter block of their own); here it is the whole 7 x 7 block.  Steps are
 * exact up to cg_relative_tolerance, so the choice changes the iteration count and not the step.  (8) Theia's intrinsics block holds the
 * whole pinhole model with the other entries set constant; here only f is a coordinate.
 */
#ifndef GSFM_BA7_H_
#define GSFM_BA7_H_

#include <stdint.h>
#include "gsfm_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSFM_BA7_ABI_VERSION 1

typedef struct gsfm_ba7_problem gsfm_ba7_problem;

int gsfm_ba7_abi_version(void);
/* gsfm_ba6_options_default (gsfm_ba_options_default with cg_relative_tolerance = 1e-14) with cg_stall_iterations = max_cg_iterations / 2 = 1000
 * where gsfm_ba.h and gsfm_ba6.h have 200 (what options == NULL means below).  At a large radius the preconditioned reduced system has the
 * seven gauge directions as eigenvalues 1e-10 to 1e-7 of the rest (held up by the damping alone), and conjugate gradients resolve them one
 * after another, each behind a run of iterations in which r.M^-1 r does not fall.  With six coordinates per camera those runs stay below 200
 * on the scenes tested; with the focal coordinate (19 instead of 13 eigenvalues below 0.1 on the same scene, the further ones carried by the
 * focal lengths) they reach 230 in a float64 host PCG and the 200 rule gave up, on the device, on a step that converges in 1600 iterations
 * (scene t of the tests under a Tukey loss at radius 1e10: DESIGN.md section 19).  The rule is there to end hopeless solves early; half of
 * the iteration budget without a quartering still does that. */
void gsfm_ba7_options_default(gsfm_ba_options* options);

/* Arguments are checked on the host before any device call as in gsfm_ba6_problem_create (a node is an orientation, a centre, a focal
 * length or a point).  focal_free: n_cams flags or NULL (all free).  A problem without a used observation is valid: its solve changes nothing. */
gsfm_status gsfm_ba7_problem_create(uint32_t n_cams, const double* intrinsics, const uint8_t* cam_estimated, const uint8_t* focal_free, uint64_t n_tracks,
                                    const uint64_t* track_ptr, const uint32_t* obs_cam, const double* obs_xy, const uint8_t* point_estimated,
                                    gsfm_ba7_problem** out);
gsfm_status gsfm_ba7_set_loss(gsfm_ba7_problem* p, const gsfm_loss_node* program, int32_t n_nodes);
/* rot_aa_inout, cam_pos_inout: n_cams x 3, focal_inout: n_cams, point_inout: n_tracks x 3: start values in, estimates out (active nodes only are
 * written; a held focal length keeps its bytes).  A focal length that is not finite or <= 0 on an active camera, free or held, is
 * GSFM_ERR_INVALID_ARG here, at gsfm_ba7_linearize and at gsfm_ba7_step_check, before any device call; inactive cameras may carry any bytes
 * and get them back.  options / summary may be NULL. */
gsfm_status gsfm_ba7_solve(gsfm_ba7_problem* p, double* rot_aa_inout, double* cam_pos_inout, double* focal_inout, double* point_inout,
                           const gsfm_ba_options* options, gsfm_ba_summary* summary);

/* ---- checks of the solve's own code (the tests compare them with a high-precision reference); every output may be NULL ---- */
gsfm_status gsfm_ba7_residuals(gsfm_ba7_problem* p, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* r_out,
                               double* rho_out);
/* gsfm_ba6_linearize with grad_focal (n_cams) and diag_cam n_cams x 49 (row-major, coordinates w, o, f); zeros on inactive nodes, and in the
 * focal entry, row and column of a camera whose focal length is held */
gsfm_status gsfm_ba7_linearize(gsfm_ba7_problem* p, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double* cost,
                               double* grad_rot, double* grad_pos, double* grad_focal, double* grad_point, double* diag_cam, double* diag_point);
/* y = Sc v (n_cams x 7, per camera w, o, f); the identity on inactive cameras and on a held focal coordinate */
gsfm_status gsfm_ba7_schur_matvec(gsfm_ba7_problem* p, const double* v, double radius, const gsfm_ba_options* options, double* y);
/* gsfm_ba6_step_check with rhs_out, yc_out n_cams x 7 and delta_focal_out (n_cams) */
gsfm_status gsfm_ba7_step_check(gsfm_ba7_problem* p, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                const gsfm_ba_options* options, double* rhs_out, double* yc_out, double* yp_out, double* delta_rot_out,
                                double* delta_pos_out, double* delta_focal_out, double* delta_point_out, double* jdelta_out, double* scal_out,
                                int32_t* info_out);
/* out_us[8] as gsfm_ba6_time_kernels, of this solver's kernels.  For tools/time_full_bundle_adjustment.py --focal. */
gsfm_status gsfm_ba7_time_kernels(gsfm_ba7_problem* p, const double* rot_aa, const double* cam_pos, const double* focal, const double* points, double radius,
                                  int32_t reps, double* out_us);
void gsfm_ba7_problem_destroy(gsfm_ba7_problem* p);

#ifdef __cplusplus
}
#endif

#endif  /* GSFM_BA7_H_ */
