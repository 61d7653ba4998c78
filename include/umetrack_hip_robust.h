/* The pose fit on 2-D keypoints in camera views under a robust loss, an entry of libumetrack_hip.so: an extension header next to
 * umetrack_hip.h, like umetrack_hip_fit.h, umetrack_hip_triangulate.h, umetrack_hip_scale.h, umetrack_hip_info.h and
 * umetrack_hip_views.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the entry that fits a pose to
 * detections some of which are grossly wrong, with the conventions of the other headers - plain device pointers and sizes, int
 * return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _ROBUST_PROTOTYPES, pinned to this header by tests/test_robust_host.py). */
#ifndef UMETRACK_HIP_ROBUST_H
#define UMETRACK_HIP_ROBUST_H

#include "umetrack_hip_views.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UT_LOSS_SQUARED 0        /* rho(s) = s: ut_fit_pose_views */
#define UT_LOSS_HUBER 1          /* rho(s) = s for s <= 1, 2 sqrt(s) - 1 above: linear in the distance beyond the scale */
#define UT_LOSS_GEMAN_MCCLURE 2  /* rho(s) = s / (1 + s): bounded, a gross outlier stops pulling */

/* ut_fit_pose_views on the cost
 *   sum_v sum_l w_vl c^2 rho(d_vl^2 / c^2),   d_vl = |project_v(landmark_l) - window_vl| in px, c = loss_scale in px,
 * which is the squared reprojection cost where d << c (csrc/fit_views_robust.hip; tests/robust_cases.py is its float64
 * restatement).  Every linearisation is a reweighted least-squares problem: observation (v, l) counts with w_vl psi(d_vl^2 / c^2),
 * psi = rho' (Huber: 1, or c / d beyond the scale; Geman-McClure: 1 / (1 + d^2 / c^2)^2), so that the gradient is the robust
 * cost's own; accept / reject, the damping and the stop rules of ut_fit_pose act on the robust cost.  A detection on the wrong
 * finger then costs one launch, not a loop of launches and read-backs around ut_fit_pose_views.
 *  Arguments as for ut_fit_pose_views, and
 *  loss        UT_LOSS_SQUARED, UT_LOSS_HUBER or UT_LOSS_GEMAN_MCCLURE
 *  loss_scale  c in px, finite and > 0: about the noise of a good detection.  Not read with UT_LOSS_SQUARED
 *  info        [n,4] or NULL: sqrt(robust cost / sum of the used weights); the largest RAW reprojection distance of a used
 *              observation in px; iterations run; status
 *  residual    out f32 [n,max_views,21] or NULL, as for ut_fit_pose_views: raw distances
 *  inlier      out f32 [n,max_views,21] or NULL: psi of every used observation at the returned pose, in (0, 1], computed from
 *              the distance that `residual` holds; 0 elsewhere.  An observation whose value is small was an outlier to the fit
 * Everything ut_fit_pose_views promises holds: its refusals (UT_FIT_REFUSED: the start comes back, or the rest pose at the
 * identity for a start whose cost is not finite), the start is required, a window at weight 0 is never read into arithmetic, a
 * pose's result does not depend on the batch it is in nor on trailing unused views, cam_rows is checked on the device (an entry
 * outside [-1, n_rows) writes nothing for its pose, `inlier` included, and gives UT_E_INVALID from this call with UT_CHECK_SYNC or
 * h == NULL, from the next ut_poll_status with UT_CHECK_DEFERRED), h may be NULL, stream ordered, no allocation.  A refused pose
 * gets inlier 0.
 * UT_LOSS_SQUARED is ut_fit_pose_views: joint_angles, wrist_xf, info and residual are bit-identical to it, and inlier is 1 at
 * every used observation of a pose that was not refused.
 * UT_E_INVALID, and nothing launched: as for ut_fit_pose_views, an unknown loss, and a loss_scale that is not finite and > 0 with
 * a robust loss.  n == 0 (with valid arguments otherwise): UT_OK, nothing launched. */
int ut_fit_pose_views_robust(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                             const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                             const float* limits, const float* init_angles, int init_ja_stride, const float* init_wrist_xf,
                             int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int loss, float loss_scale,
                             int n, float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info,
                             float* residual, float* inlier, void* stream);

#ifdef __cplusplus
}
#endif
#endif
