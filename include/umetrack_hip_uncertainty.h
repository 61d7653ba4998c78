/* How well a pose fitted in the views is known, an entry of libumetrack_hip.so: an extension header next to umetrack_hip.h, like
 * umetrack_hip_fit.h, umetrack_hip_triangulate.h, umetrack_hip_scale.h, umetrack_hip_info.h, umetrack_hip_views.h,
 * umetrack_hip_robust.h and umetrack_hip_views_scale.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the entry that gives a pose its
 * information matrix and its covariances, with the conventions of the other headers - plain device pointers and sizes, int
 * return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _UNCERTAINTY_PROTOTYPES, pinned to this header by tests/test_uncertainty_host.py). */
#ifndef UMETRACK_HIP_UNCERTAINTY_H
#define UMETRACK_HIP_UNCERTAINTY_H

#include "umetrack_hip_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UT_COV_OK 1        /* every output holds what it is documented to hold */
#define UT_COV_SINGULAR 2  /* the detections (and the prior) leave a direction of the pose free: sigmas and covariances are +inf */
#define UT_COV_REFUSED 4   /* = UT_FIT_REFUSED, and for the fit's reasons: every output of the pose is 0 */
#define UT_COV_MIN_PIVOT 1.52587890625e-05f /* 2^-16: a pivot of the unit-diagonal matrix at or below it counts as 0 */

/* The information of a pose under the cost of ut_fit_pose_views_robust, in one launch that changes nothing
 * (csrc/pose_info_views.hip; tests/uncertainty_cases.py is its float64 restatement):
 *   H = sum_v sum_l w_vl psi_vl J_vl^T J_vl  (+ the prior),
 * the normal matrix the fit's solver forms at this pose - its reduction to 63 rows, the semidefinite 3 x 3 factor per landmark
 * and that factor's pivot floor included - on the solver's 26 parameters: 20 joint angle increments (rad), a rotation increment
 * about `pivot` in world axes (rad), a translation in target units.  psi is the loss's weight at the pose's own residuals
 * (1 for UT_LOSS_SQUARED).  H^-1 is the Gauss-Newton covariance: it has no second-order term, under a robust loss it is that of
 * the reweighted least-squares problem, and it means something at a minimum of the cost - at the pose a fit returned.
 *  hand_model .. table_kind, mirror, t_scale, loss, loss_scale   exactly as for ut_fit_pose_views_robust
 *  weights       informations in px^-2: with w = 1 / sigma^2 of each detection the covariances are absolute, with unit weights
 *                (NULL) they are per px^2 of detection noise
 *  angle_sigma   f32 [n_models,20] or NULL: the standard deviation in rad of a Gaussian prior on each joint angle, each finite
 *                and > 0 with a finite 1 / sigma^2 in fp32 (any other value refuses the pose); 1 / sigma^2 is added to H's
 *                diagonal.  The prior lives here and not in the fit: for an angle the detections observe it is negligible, for
 *                one they do not observe it is the whole answer
 *  joint_angles  [n,22] rows ja_stride floats apart, wrist_xf [n,4,4] (12 floats read) rows xf_stride floats apart: the pose,
 *                read the way the fit reads its start, so pose records and the fit's own outputs are consumed in place
 * There is no `limits` argument: the pose is taken as given, and the result is the information of the UNCONSTRAINED
 * linearisation - an angle that the fit left on its box has a one-sided uncertainty that this does not describe.
 * Outputs, each f32 and each may be NULL (not all five):
 *  pose_info     [n,351]: the lower triangle of H, row-major (entry (i, j <= i) at i (i + 1) / 2 + j)
 *  pivot         [n,3]: the weighted centroid of the pose's landmarks (weights sum_v w_vl) that the rotation increment turns about
 *  param_sigma   [n,26]: sqrt(diag H^-1)
 *  landmark_cov  [n,21,6]: (xx, yx, yy, zx, zy, zz) of G_l H^-1 G_l^T in target units^2, G_l the landmark's 3 x 26 world Jacobian
 *                (the solver's rows before whitening).  Written for all 21 landmarks: an unobserved one gets the uncertainty that
 *                the pose gives it
 *  info          [n,4]: sqrt(cost / sum of the used weights) at the pose, as the fit's info[0]; the square root of the largest
 *                landmark covariance trace; the smallest pivot of the scaled factor; status UT_COV_*
 * Arithmetic: H is scaled to unit diagonal (Jacobi) and factorised by Cholesky in fp32; a pivot is the diagonal entry of the
 * Schur complement, the square of the factor's diagonal.  A diagonal entry of H that is 0 (pivot 0), or a pivot <=
 * UT_COV_MIN_PIVOT, gives UT_COV_SINGULAR: the factorisation stops there, info[2] is the smallest pivot seen up to and including
 * that one, pose_info, pivot and info[0] are written as usual, param_sigma is +inf, landmark_cov is +inf at xx / yy / zz and 0
 * elsewhere, info[1] is +inf - a caller who skips the status reads "unknown", not "certain".
 * UT_COV_REFUSED: ut_fit_pose_views' refusals (a negative or non-finite weight of a seen view, a non-finite window at a positive
 * weight, fewer than 3 landmarks with a used observation, a cost at the pose that is not finite) and a bad angle_sigma; all
 * outputs of the pose are 0 but info[3].
 * As for the fit: a window at weight 0 is never read into arithmetic, a pose's result does not depend on the batch it is in nor
 * on trailing unused views, cam_rows is checked on the device (an entry outside [-1, n_rows) writes nothing for its pose and gives
 * UT_E_INVALID from this call with UT_CHECK_SYNC or h == NULL, from the next ut_poll_status with UT_CHECK_DEFERRED), h may be NULL,
 * stream ordered, no allocation, capturable with deferred checks.
 * UT_E_INVALID, and nothing launched: as for ut_fit_pose_views_robust, a null pose pointer, all five outputs NULL.  n == 0 (with
 * valid arguments otherwise): UT_OK, nothing launched. */
int ut_pose_information_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                              const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                              const float* angle_sigma, const float* joint_angles, int ja_stride, const float* wrist_xf,
                              int xf_stride, const int64_t* mirror, float t_scale, int loss, float loss_scale, int n,
                              float* pose_info, float* pivot, float* param_sigma, float* landmark_cov, float* info,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
