/* Fitted poses smoothed over a sequence, an entry of libumetrack_hip.so: an extension header next to umetrack_hip.h, like
 * umetrack_hip_fit.h, umetrack_hip_triangulate.h, umetrack_hip_scale.h, umetrack_hip_info.h, umetrack_hip_views.h,
 * umetrack_hip_robust.h, umetrack_hip_views_scale.h and umetrack_hip_uncertainty.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the entry that combines the poses of
 * consecutive frames by their information matrices, with the conventions of the other headers - plain device pointers and sizes,
 * int return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _SMOOTH_PROTOTYPES, pinned to this header by tests/test_smooth_host.py). */
#ifndef UMETRACK_HIP_SMOOTH_H
#define UMETRACK_HIP_SMOOTH_H

#include "umetrack_hip_uncertainty.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UT_SMOOTH_OK 1        /* the frame holds the smoothed pose */
#define UT_SMOOTH_GAP 8       /* set together with UT_SMOOTH_OK: the frame measured nothing (weight 0 or H = 0), the motion model filled it in */
#define UT_SMOOTH_SINGULAR 2  /* no frame of the sequence observes some direction: poses copied through, sigmas +inf */
#define UT_SMOOTH_REFUSED 4   /* = UT_FIT_REFUSED: poses copied through, sigmas 0 */
#define UT_SMOOTH_WORK 408    /* floats of workspace per frame */

/* The maximum a-posteriori sequence of poses under a Gauss-Markov motion model, given every frame's fitted pose and the
 * information matrix ut_pose_information_views gave it (csrc/smooth.hip; tests/smooth_cases.py holds the float64 restatement,
 * which is the definition: a dense solve of the block-tridiagonal system).  No camera model, no projection, no fit.
 *
 * Frame t of sequence s is row s * n_frames + t of every per-frame array.  It has the fitted pose (angles th_t, wrist [R_t | t_t],
 * translation in target units / t_scale), H_t (pose_info, the packed lower triangle [351]), c_t (pivot) and a weight f_t >= 0
 * (frame_weight, NULL = 1) that multiplies H_t.  A frame with f_t = 0 or H_t = 0 is a GAP: its pose is only the point of
 * linearisation (H_t and c_t are not read into arithmetic at f_t = 0, and the frame's rotation increment turns about the body
 * point).  A pose that ut_pose_information_views refused has H = 0; one it called UT_COV_SINGULAR has a semidefinite H that is
 * used as it is.
 *
 * The unknown of a frame is a correction delta_t in the fit's chart: th = th_t + delta_th (20), R = E(omega) R_t,
 * t t_scale = E(omega) (t_t t_scale - c_t) + c_t + tau.  The motion model speaks about the body-fixed point b (`centre`,
 * [n_seq,3] in the PROPER wrist frame - x negated for a wrist with determinant < 0 - in target units, NULL = the wrist's origin),
 * x_t = R_t b + t_t t_scale.  With a_t = x_t - c_t and B_t = I_26 but for the block (rows 23..25, columns 20..22) = -[a_t]x:
 *   u_t = B_t delta_t,   H'_t = f_t B_t^-T H_t B_t^-1   (B_t^-1 has +[a_t]x in that block),
 *   d_t = (wrap(th_t+1 - th_t) into (-pi, pi], log(R_t+1 R_t^T) as a rotation vector in world axes, x_t+1 - x_t),
 *   W = diag(1 / q), q = step_var [n_var,26], n_var 1 or n_seq: the random walk's variance per frame step in rad^2 (20 angles),
 *   rad^2 (rotation), target units^2 (body point), each finite and > 0 with a finite reciprocal in fp32;
 *   minimise  sum_t u_t^T H'_t u_t + sum_t (d_t + u_t+1 - u_t)^T W (d_t + u_t+1 - u_t).
 * ONE linear solve: it is not iterated, and it is first order in omega (the rotation part of d_t and u_t add as vectors).  The
 * solution goes back through delta_t = B_t^-1 u_t and the chart; angles are wrapped into (-pi, pi] as the fits wrap them, angles 20
 * and 21 are copied, the wrist's bottom row (0 0 0 1) is written when xf_out_stride >= 16.
 *
 * Arithmetic (fp32): a forward information filter  P_0 = H'_0, eta_0 = 0, S_t-1 = P_t-1 + W, M_t = W S_t-1^-1 P_t-1 (this
 * product, symmetrised - never W - W S^-1 W, which cancels for small q), eta_t = W S_t-1^-1 (eta_t-1 - P_t-1 d_t-1), P_t = M_t +
 * H'_t;  backward  u_T-1 = P_T-1^-1 eta_T-1, u_t = S_t^-1 (eta_t + W (u_t+1 + d_t));  marginal covariances C_T-1 = P_T-1^-1,
 * C_t = S_t^-1 + S_t^-1 W C_t+1 W S_t^-1.  Every matrix is factorised by Cholesky after scaling to unit diagonal, with the pivot
 * rule of ut_pose_information_views: a pivot is the diagonal of the Schur complement, one <= UT_COV_MIN_PIVOT counts as 0.  S_t is
 * positive definite by construction; P_T-1 fails the rule when no frame observes some direction: UT_SMOOTH_SINGULAR.
 *
 *  joint_angles [.,22] rows ja_stride >= 22 floats apart, wrist_xf [.,4,4] (12 floats read) rows xf_stride >= 12 floats apart:
 *                pose records and a fit's outputs are read in place
 *  pose_info [.,351], pivot [.,3]   as ut_pose_information_views writes them
 *  frame_weight  [n_seq * n_frames] or NULL
 *  lengths       i32 [n_seq] or NULL (= n_frames): frames at or past the length are copied through with status 0, sigma 0 and
 *                info 0.  A length outside [0, n_frames] refuses the sequence on the device
 *  centre        [n_seq,3] or NULL
 *  workspace     f32 [n_seq * n_frames, UT_SMOOTH_WORK]: what the forward pass leaves for the backward pass.  Because of it the
 *                outputs may be the inputs' own buffers (same strides): a frame is read before it is written
 * Outputs:
 *  joint_angles_out [.,22] / wrist_xf_out [.,4,4], rows ja_out_stride >= 22 / xf_out_stride >= 12 floats apart
 *  param_sigma   [.,26] or NULL: sqrt(diag C_t), in the chart of u - its translation (23..25) is that of the body point `centre`,
 *                not of `pivot`
 *  info          [.,4] or NULL: sqrt(u_t^T H'_t u_t), how many of the fit's own sigmas the smoothing moved the frame (large: a
 *                fit that disagrees with its neighbours); sqrt(m_t^T W m_t) of the smoothed step m_t = d_t + u_t+1 - u_t, 0 on the
 *                last frame; the smallest scaled pivot met at the frame (of S_t, on the last frame of P_T-1); the status
 * UT_SMOOTH_REFUSED (whole sequence; outputs are the inputs, sigma 0, info 0 0 0 status): a pose inside the length that is not
 * finite, an H or pivot that is not finite at a positive weight, a weight that is negative or not finite, a bad step_var, a bad
 * length.  UT_SMOOTH_SINGULAR (whole sequence): outputs are the inputs, sigma +inf, info 0 0 pivot status.
 * A sequence's result does not depend on the batch it is in, nor on the frames behind its length.  h may be NULL, stream ordered,
 * no allocation, no host synchronisation, capturable.
 * UT_E_INVALID, and nothing launched: a null required pointer (joint_angles, wrist_xf, pose_info, pivot, step_var, workspace,
 * joint_angles_out, wrist_xf_out), a stride below 22 / 12, n_var not 1 or n_seq, n_frames < 1, n_seq < 0, a t_scale that is not
 * positive and finite; ut_last_error names the argument.  n_seq == 0 (with valid arguments otherwise): UT_OK, nothing launched.
 * Not built: constant-velocity models, uneven time steps, a gradient term for fits that did not converge.  A sliding window over
 * the last L frames is a call with n_frames = L. */
int ut_smooth_pose_sequence(ut_handle h, const float* joint_angles, int ja_stride, const float* wrist_xf, int xf_stride,
                            const float* pose_info, const float* pivot, const float* frame_weight, const int32_t* lengths,
                            const float* centre, const float* step_var, int n_var, float t_scale, int n_seq, int n_frames,
                            float* workspace, float* joint_angles_out, int ja_out_stride, float* wrist_xf_out, int xf_out_stride,
                            float* param_sigma, float* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
