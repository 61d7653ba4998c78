/* Pose fitting entry of libumetrack_hip.so: an extension header next to umetrack_hip.h.
 *
 * umetrack_hip.h is the core boundary: its list of entries is closed (tests/test_host_logic.py pins every declaration of it to
 * the binding's core prototype table, by name and by count).  Entries added to the library after that live in headers of
 * their own, like this one, with the same conventions - plain device pointers and sizes, int return codes of umetrack_hip.h,
 * ut_last_error for the text, stream ordered - and a prototype table of their own in the binding
 * (absolutetrack_amd/_native.py: _EXTENSION_PROTOTYPES, pinned to this header by tests/test_fit_host.py). */
#ifndef UMETRACK_HIP_FIT_H
#define UMETRACK_HIP_FIT_H

#include "umetrack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The inverse of ut_fk (lib/common/hand_skinning.py:189-209, skin_landmarks): the pose - 20 joint angles and a rigid wrist
 * transform - whose 21 landmarks meet given targets, for a batch of poses in one launch.  The reference has no counterpart.
 * Levenberg-Marquardt in fp32 on the angles and a wrist increment, analytic Jacobian, a step accepted only when the weighted
 * cost sum_l w_l |landmark_l - target_l|^2 goes down (csrc/fit.hip; tests/fit_cases.py is its float64 restatement).
 *  hand_model, n_models, mirror, t_scale: as for ut_fk of umetrack_hip.h (n_models in {1, n}; t_scale positive and finite)
 *  targets       row i starts target_stride floats after row i - 1 and begins with its 21 points (target_stride >= 63): a
 *                packed [n,21,3] array, or the keypoints inside records, read in place; in the unit of the model
 *  weights       [n,21] >= 0, or NULL = all 1.  The target of a landmark of weight 0 is never read into arithmetic: a NaN
 *                there changes nothing
 *  limits        [n_models,20,2] (lower, upper) or NULL.  With limits every trial angle - the start too - is clamped to the
 *                box before the cost is evaluated and the output angles lie inside it; without, output angles are wrapped
 *                to (-pi, pi]
 *  init_angles, init_wrist_xf  both NULL: cold start, the rest pose aligned to the targets by a weighted Kabsch fit.  Both
 *                given ([n] rows of >= 22 / >= 12 floats with their strides, e.g. last frame's pose records): warm start.  A
 *                warm start far from the answer can end in a local minimum; that is the caller's to judge from `info`
 *  max_iters     1..256 iterations (one solve and one trial each) per pose
 *  joint_angles  out, rows of ja_stride >= 22 floats: 22 angles; angles 20, 21 do not move the landmarks and are 0 on a cold
 *                start, copied from the start otherwise
 *  wrist_xf      out, rows of xf_stride >= 12 floats: the PROPER rigid transform that pose records hold, row major (the mirror
 *                is applied by the consumer, as ut_fk does), translation in the unit of the targets / t_scale; with
 *                xf_stride >= 16 the bottom row 0 0 0 1 is written as well.  Both outputs may be pose records written in
 *                place, and may be the start's own buffers.  ut_fk(hand_model, joint_angles, wrist_xf, mirror, t_scale)
 *                reproduces the targets
 *  info          [n,4] or NULL: weighted rms residual sqrt(cost / sum w), largest residual of a weighted landmark, iterations
 *                run, status
 * Status bits: UT_FIT_CONVERGED the last step and its relative cost decrease were below the thresholds, or a rejected trial
 * left the cost where it was to fp32 resolution (noisy targets: the residual cannot go lower); UT_FIT_AT_MAX_ITERS
 * stopped at max_iters (the best pose found is returned); UT_FIT_REFUSED this pose's input was refused - fewer than 3
 * landmarks of non-zero weight, a negative or non-finite weight, a non-finite target of a weighted landmark - and its outputs
 * are the start as given (the rest pose at the identity on a cold start, or when the start itself is not finite): finite.
 * A failed factorisation or a non-finite trial is a rejected step, never a NaN in the output.  A pose's result does not
 * depend on the batch it is in.  Stateless: h may be NULL.  Stream ordered, no allocation, no synchronisation: capturable.
 * UT_E_INVALID, and nothing launched: a null hand_model / targets / joint_angles / wrist_xf, only one of the two init
 * pointers, target_stride < 63, an angle stride < 22, a wrist stride < 12, max_iters outside 1..256, n_models not in
 * {1, n}, n < 0, a t_scale that is not positive and finite. */
enum { UT_FIT_CONVERGED = 1, UT_FIT_AT_MAX_ITERS = 2, UT_FIT_REFUSED = 4 };
int ut_fit_pose(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                const float* weights, const float* limits, const float* init_angles, int init_ja_stride,
                const float* init_wrist_xf, int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int n,
                float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
