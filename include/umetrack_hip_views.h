/* The pose fit on 2-D keypoints in camera views, an entry of libumetrack_hip.so: an extension header next to umetrack_hip.h, like
 * umetrack_hip_fit.h, umetrack_hip_triangulate.h, umetrack_hip_scale.h and umetrack_hip_info.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the entry that fits a pose to the
 * detections themselves, with the conventions of the other headers - plain device pointers and sizes, int return codes of
 * umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _VIEWS_PROTOTYPES, pinned to this header by tests/test_views_host.py). */
#ifndef UMETRACK_HIP_VIEWS_H
#define UMETRACK_HIP_VIEWS_H

#include "umetrack_hip_fit.h"
#include "umetrack_hip_triangulate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The pose whose landmarks, projected into the views, meet the detections: the minimum of
 *   sum_v sum_l w_vl |project_v(landmark_l) - window_vl|^2
 * over 20 joint angles and the wrist, through the exact forward model of ut_project_points / ut_triangulate_points
 * (csrc/fit_views.hip; tests/views_cases.py is its float64 restatement).  Where the chain ut_triangulate_points[_info] ->
 * ut_fit_pose[_info] drops every landmark that fewer than two cameras see, here every detection counts: a hand that one camera
 * alone sees can be fitted - its known size fixes its depth - and a hand that one camera sees only partly keeps what that
 * camera sees.  It is ut_fit_pose_info with the factor derived again at every accepted state: solver, constants, stop rules,
 * status bits (UT_FIT_*), pose outputs and their in-place use are ut_fit_pose's.
 *  hand_model, n_models, limits, mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride   as for ut_fit_pose
 *  window      f64 [n,max_views,21,2] px: the layout ut_project_points writes
 *  weights     f32 [n,max_views,21], each >= 0, or NULL = all 1
 *  cam_rows, table, n_rows, table_kind   as for ut_triangulate_points: i32 [n,max_views] rows of `table`, -1 = unused view;
 *              UT_CAMERA_FISHEYE62 rows of 32 doubles or UT_CAMERA_PINHOLE crop-camera rows of 24 doubles.  The cameras' world
 *              is in target units: model units x t_scale
 *  max_views   1..UT_TRI_MAX_VIEWS.  A pose's result does not depend on trailing unused views
 *  init_angles, init_wrist_xf   the start, REQUIRED: there is no cold start, because there are no 3-D targets to align the rest
 *              pose to.  The two intended starts are the previous frame's pose, and the chain ut_triangulate_points ->
 *              ut_fit_pose on the landmarks that can be triangulated
 *  info        [n,4] or NULL: sqrt(cost / sum of the used weights) - px at unit weights -; the largest reprojection distance of a
 *              used observation in px; iterations run; status
 *  residual    out f32 [n,max_views,21] or NULL: the reprojection distance in px of every used observation at the returned pose,
 *              0 elsewhere - a caller rejects an outlier from this and calls again with its weight set to 0
 * An observation is used when its view's cam_rows entry is >= 0, its weight is finite and > 0 and its window is finite.  The
 * window of a weight-0 observation is never read into arithmetic: a NaN there changes nothing.  The weight of a view whose
 * cam_rows entry is -1 is not read.
 * UT_FIT_REFUSED: a negative or non-finite weight of a seen view, a non-finite window at a positive weight, fewer than 3 landmarks
 * with a used observation - the pose is then the start as given - or a start whose cost is not finite (a landmark that cannot be
 * projected into a used view, or that lies in front of UT_TRI_NEAR_Z of a used pinhole view): outputs then as for ut_fit_pose's
 * non-finite start, the rest pose at the identity.  info is (0, 0, 0, UT_FIT_REFUSED), residuals 0.
 * A trial in which a used observation is not finite or crosses the near plane of a used pinhole view is a rejected step, never a
 * NaN in the output.  The wrist increment turns about the weighted centroid of the start's landmarks (weight sum_v w_vl), and
 * the translation's step tolerance scales with their extent.
 * A pose's result does not depend on the batch it is in.  Stateless: h may be NULL.  Stream ordered, no allocation.  cam_rows
 * is checked on the device: an entry outside [-1, n_rows) writes nothing for its pose and gives UT_E_INVALID ("index check:
 * ...") - from this call with UT_CHECK_SYNC or h == NULL, from the next ut_poll_status with UT_CHECK_DEFERRED, where nothing
 * synchronises and the launch is capturable.
 * UT_E_INVALID, and nothing launched: as for ut_fit_pose (without its targets) and ut_triangulate_points (without its outputs),
 * and a null init_angles or init_wrist_xf.  n == 0 (with valid arguments otherwise): UT_OK, nothing launched. */
int ut_fit_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                      const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind, const float* limits,
                      const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                      const int64_t* mirror, float t_scale, int max_iters, int n, float* joint_angles, int ja_stride,
                      float* wrist_xf, int xf_stride, float* info, float* residual, void* stream);

#ifdef __cplusplus
}
#endif
#endif
