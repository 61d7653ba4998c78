/* Hand scale entries of libumetrack_hip.so: an extension header next to umetrack_hip.h, like umetrack_hip_fit.h (same
 * conventions: plain device pointers and sizes, int return codes of umetrack_hip.h, ut_last_error for the text, stream
 * ordered; the binding keeps a prototype table of its own for it, absolutetrack_amd/_native.py: _SCALE_PROTOTYPES, pinned to
 * this header by tests/test_scale_host.py). */
#ifndef UMETRACK_HIP_SCALE_H
#define UMETRACK_HIP_SCALE_H

#include "umetrack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A hand model whose lengths fit the person in front of the cameras, from keypoints.  The reference gets one only through
 * its network (run_eval_unknown_skeleton.py:55-76: the mean of predicted scales, applied by scaled_hand_model).  Scale s means
 * exactly hand.scaled_hand_model(model, s): joint_rest_positions and landmark_rest_positions times s in fp32, nothing else.
 *
 * ut_fit_pose_scale is ut_fit_pose (umetrack_hip_fit.h) with sigma = ln s as a 27th parameter (csrc/fit_scale.hip;
 * tests/scale_cases.py is its float64 restatement).  Everything ut_fit_pose documents holds unchanged - hand_model, targets and
 * their stride, weights (the target of a landmark of weight 0 is never read), limits, the two init pointers, mirror, t_scale,
 * max_iters, the in-place outputs and their strides, the refusal rules - and in addition:
 *  init_scale    [n] or NULL = 1: the scale the fit starts from; a cold start is the rest pose of the model at this scale.  A
 *                non-finite one, or one outside [UT_SCALE_MIN, UT_SCALE_MAX], refuses that pose
 *  scale_mode    UT_SCALE_FREE: the scale is fitted, every trial clamped to [UT_SCALE_MIN, UT_SCALE_MAX].  UT_SCALE_FIXED: the
 *                scale stays init_scale, bit for bit - ut_fit_pose on the scaled model, without building one blob per pose
 *  scale         out [n]: the fitted scale; 1 for a refused pose.  ut_fk on the blob of scaled_hand_model(model, scale[i]) with
 *                the output pose reproduces the residual the solver saw
 *  info          [n,6] or NULL: weighted rms residual, largest residual of a weighted landmark, iterations, status, scale
 *                information, 0 (reserved).  The scale information is 1 / variance of ln s per unit^2 of target noise with pose
 *                and wrist marginalised: the Schur complement of sigma in J^T W J + UT_SCALE_INFO_LAMBDA D (D: its floored
 *                diagonal) at the returned state.  0 when that matrix cannot be factorised, for a refused pose and in
 *                UT_SCALE_FIXED mode.  A hand seen only at its wrist and fingertips says next to nothing about its scale
 *                (bent fingers explain a short hand): its information is small, and the pool weighs it accordingly
 * Status bits: UT_FITS_CONVERGED, UT_FITS_AT_MAX_ITERS, UT_FITS_REFUSED as UT_FIT_* of ut_fit_pose (a small step here also
 * needs |delta sigma| below the step tolerance); UT_FITS_AT_BOUND a free fit ended at UT_SCALE_MIN or UT_SCALE_MAX.
 * A pose's result does not depend on the batch it is in.  Stateless: h may be NULL.  Stream ordered, no allocation, no
 * synchronisation: capturable.  UT_E_INVALID, and nothing launched: what ut_fit_pose lists, an unknown scale_mode, a null
 * scale.  n == 0 is UT_OK.
 *
 * ut_pool_scale turns the per-pose scales of a free pass into one per group of group_size consecutive poses, in fp64: a
 * pose is used when its status has UT_FITS_CONVERGED and neither UT_FITS_REFUSED nor UT_FITS_AT_BOUND and its information I
 * is finite and > 0.
 *  scale, info   [n_groups * group_size], [n_groups * group_size, 6]: the outputs of ut_fit_pose_scale
 *  group         out [n_groups,4]: scale = exp(sum I ln s / sum I); sigma = 1 / sqrt(sum I), the standard deviation of
 *                ln(scale) per unit of target noise; scatter = sqrt(sum I (ln s - ln scale)^2 / max(n_used - 1, 1)), in
 *                target units the per-landmark noise that would explain how much the poses disagree (bone proportions that
 *                differ from the model's show up here); n_used.  A group without a usable pose: 1, +inf, 0, 0
 *  pose_scale    out [n_groups * group_size] or NULL: the group's scale for each of its poses - the init_scale of a following
 *                UT_SCALE_FIXED pass
 * A group's row does not depend on the other groups.  Stateless, stream ordered, no allocation, no synchronisation: the chain
 * free pass -> pool -> fixed pass is capturable.  UT_E_INVALID, and nothing launched: a null scale / info / group,
 * n_groups < 0, group_size < 1.  n_groups == 0 is UT_OK. */
enum { UT_SCALE_FREE = 0, UT_SCALE_FIXED = 1 };
enum { UT_FITS_CONVERGED = 1, UT_FITS_AT_MAX_ITERS = 2, UT_FITS_REFUSED = 4, UT_FITS_AT_BOUND = 8 };
#define UT_SCALE_MIN 0.25f
#define UT_SCALE_MAX 4.0f
#define UT_SCALE_INFO_LAMBDA 1e-6f
int ut_fit_pose_scale(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                      const float* weights, const float* limits, const float* init_scale, int scale_mode,
                      const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                      const int64_t* mirror, float t_scale, int max_iters, int n,
                      float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride,
                      float* scale, float* info, void* stream);
int ut_pool_scale(ut_handle h, const float* scale, const float* info, int n_groups, int group_size,
                  float* group, float* pose_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
