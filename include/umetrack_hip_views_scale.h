/* The hand's scale from 2-D keypoints in camera views, an entry of libumetrack_hip.so: an extension header next to
 * umetrack_hip.h, like umetrack_hip_fit.h, umetrack_hip_triangulate.h, umetrack_hip_scale.h, umetrack_hip_info.h,
 * umetrack_hip_views.h and umetrack_hip_robust.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the entry that fits a pose AND the
 * hand's scale to the detections themselves, with the conventions of the other headers - plain device pointers and sizes, int
 * return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _VIEWS_SCALE_PROTOTYPES, pinned to this header by tests/test_views_scale_host.py). */
#ifndef UMETRACK_HIP_VIEWS_SCALE_H
#define UMETRACK_HIP_VIEWS_SCALE_H

#include "umetrack_hip_robust.h"
#include "umetrack_hip_scale.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ut_fit_pose_views_robust (umetrack_hip_robust.h) with sigma = ln s as a 27th parameter, as ut_fit_pose_scale
 * (umetrack_hip_scale.h) is to ut_fit_pose (csrc/fit_views_scale.hip; tests/views_scale_cases.py is its float64 restatement).
 * The chain it is made for: detections -> a start from the 3-D chain (ut_triangulate_points, ut_fit_pose_scale) -> a
 * UT_SCALE_FREE pass here -> ut_pool_scale -> a UT_SCALE_FIXED pass here at the pooled scale.
 *
 * Views arguments.  hand_model, window, weights, cam_rows, max_views, table, n_rows, table_kind, limits, the two init pointers
 * (required: there is no cold start), mirror, t_scale, max_iters, loss, loss_scale (UT_LOSS_*; UT_LOSS_SQUARED is the default
 * use), the in-place pose outputs and their strides, residual and inlier mean what they mean for ut_fit_pose_views_robust, and
 * what it promises holds: its refusals, a window at weight 0 is never read into arithmetic, a pose's result does not depend on
 * the batch it is in nor on trailing unused views, cam_rows is checked on the device (an entry outside [-1, n_rows) writes
 * nothing for its pose, `scale` included, and gives UT_E_INVALID from this call with UT_CHECK_SYNC or h == NULL, from the next
 * ut_poll_status with UT_CHECK_DEFERRED), h may be NULL, stream ordered, no allocation, capturable with deferred checks.
 *
 * Scale arguments.  As for ut_fit_pose_scale: scale s means exactly hand.scaled_hand_model(model, s);
 *  init_scale    [n] or NULL = 1: the scale of the start.  A non-finite one, or one outside [UT_SCALE_MIN, UT_SCALE_MAX],
 *                refuses that pose
 *  scale_mode    UT_SCALE_FREE: the scale is fitted, every trial clamped to [UT_SCALE_MIN, UT_SCALE_MAX].  UT_SCALE_FIXED: the
 *                scale stays init_scale, bit for bit - ut_fit_pose_views_robust on the scaled model, without one blob per pose
 *  scale         out [n]: the fitted scale; 1 for a refused pose (a start whose cost is not finite gives the rest pose at the
 *                identity and scale 1)
 *  info          [n,6] or NULL, the row layout ut_pool_scale reads: sqrt(cost / sum of the used weights) in px (the robust
 *                cost's rms under a robust loss); the largest raw reprojection distance in px; iterations; status bits
 *                UT_FITS_* (UT_FITS_AT_BOUND: a free fit ended at UT_SCALE_MIN or UT_SCALE_MAX); scale information; 0
 * The scale information is the Schur complement of sigma in A + UT_SCALE_INFO_LAMBDA D at the returned state (A the normal
 * matrix of the weighted reprojection residuals, D its floored diagonal): 1 / variance of ln s per px^2 of detection noise at
 * unit weights, pose and wrist marginalised.  0 in UT_SCALE_FIXED mode, for a refused pose and when the matrix cannot be
 * factorised.
 *
 * ONE CAMERA CANNOT SEE THE HAND'S SIZE.  Scaling the world about a central camera leaves every projection unchanged, so a
 * UT_SCALE_FREE fit on one view converges (rms 3e-7 px on exact windows) to a scale that means nothing: in the float64
 * restatement it was off by up to 0.18 with an information of 0.19 - 1.5, against 4.4e3 - 2.3e4 for the same hands in two views.
 * The information is how the caller and ut_pool_scale know - a one-view pose pooled with two-view poses does not move the pooled
 * scale - and UT_SCALE_FIXED is what one-view frames are for.
 *
 * UT_E_INVALID, and nothing launched: everything ut_fit_pose_views_robust lists, an unknown scale_mode, a null scale.  n == 0
 * (with valid arguments otherwise): UT_OK, nothing launched. */
int ut_fit_pose_views_scale(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                            const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                            const float* limits, const float* init_scale, int scale_mode,
                            const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                            const int64_t* mirror, float t_scale, int max_iters, int loss, float loss_scale, int n,
                            float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* scale, float* info,
                            float* residual, float* inlier, void* stream);

#ifdef __cplusplus
}
#endif
#endif
