/* A start for the pose fits in the views that needs nothing but the detections, and the selection among fitted candidates: entries
 * of libumetrack_hip.so in an extension header next to umetrack_hip.h, like umetrack_hip_views.h and umetrack_hip_smooth.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  The conventions are those of the other headers - plain
 * device pointers and sizes, int return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - with a prototype
 * table of their own in the binding (absolutetrack_amd/_native.py: _START_PROTOTYPES, pinned to this header by
 * tests/test_start_host.py). */
#ifndef UMETRACK_HIP_START_H
#define UMETRACK_HIP_START_H

#include "umetrack_hip_views.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UT_START_MAX_SEEDS 64

/* Starts for ut_fit_pose_views[_robust] from the detections alone: generalised PnP by orthogonal iteration over a bank of finger
 * poses and a set of rotation seeds (csrc/start_views.hip; tests/start_cases.py is its float64 restatement).
 * For bank pose k the hand is rigid: p_l are the landmarks of bank_angles[k] (clamped to `limits`) under the identity wrist,
 * column 0 negated for a mirrored hand.  Every used observation (v, l) is a ray with the camera centre o_v as origin and the unit
 * direction d_vl of ut_triangulate_points' start rays (the reference's radial-only five-step unprojection), A_vl = I - d d^T, and
 *   sum_vl w_vl |A_vl (R p_l + t - o_v)|^2
 * is minimised over a proper rotation R and a translation t: given R, t = -(sum w A)^-1 sum w A (R p_l - o_v); given (R, t) the
 * foot points q_vl = o_v + d d^T (R p_l + t - o_v); the next R is the weighted Kabsch rotation of p_l -> q_vl.  `iters` such
 * rounds, no stop rule, then t once more.  Seed s starts at R = R_eye->world(first view with a used observation) x seeds[s].
 * A seed's score is the squared cost of ut_fit_pose_views at its end, through the exact forward projection on R p_l + t in
 * float64, +inf where a used observation cannot be projected or lies in front of UT_TRI_NEAR_Z of a used pinhole view.  Per (hand,
 * bank pose) the seed with the lowest score wins, the lowest index among equals.
 *  hand_model, n_models, window, weights, cam_rows, max_views, table, n_rows, table_kind, limits, mirror, t_scale, n
 *              as for ut_fit_pose_views, and so are the rules for used observations
 *  bank_angles f32 [n_bank,20], n_bank >= 1
 *  seeds       f64 [n_seeds,9] row-major proper rotations, 1 <= n_seeds <= UT_START_MAX_SEEDS
 *  iters       1..256
 *  joint_angles, wrist_xf   out, n * n_bank rows with the strides given in floats (>= 22 / >= 12): row i * n_bank + k is the start
 *              of hand i from bank pose k, in the layout ut_fit_pose_views takes as init_*: the clamped bank angles and two zeros;
 *              [R | t / t_scale], and row 3 = (0, 0, 0, 1) when xf_stride >= 16
 *  info        [n * n_bank,4] or NULL: sqrt(score / sum of the used weights) px, the largest reprojection distance px, the winning
 *              seed's index, status 0
 * UT_FIT_REFUSED: a negative or non-finite weight of a seen view, a non-finite window at a positive weight, fewer than 3 landmarks
 * with a used observation, a singular sum w A (all rays parallel), or every seed scoring +inf: the row is the clamped bank pose
 * at the identity wrist, info (0, 0, -1, UT_FIT_REFUSED).
 * A row's result does not depend on the batch it is in, nor on trailing unused views.  Stateless: h may be NULL.  Stream ordered,
 * no allocation.  cam_rows is checked on the device as for ut_fit_pose_views: an entry outside [-1, n_rows) writes nothing for its
 * hand and gives UT_E_INVALID ("index check: ...") - from this call with UT_CHECK_SYNC or h == NULL, from the next ut_poll_status
 * with UT_CHECK_DEFERRED, where nothing synchronises and the launch is capturable.
 * UT_E_INVALID, and nothing launched: a null required pointer, a bad table_kind, max_views, n_rows, n_models, n_bank, n_seeds,
 * iters, stride or t_scale.  n == 0 (with valid arguments otherwise): UT_OK, nothing launched. */
int ut_start_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                        const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                        const float* limits, const float* bank_angles, int n_bank, const double* seeds, int n_seeds,
                        const int64_t* mirror, float t_scale, int iters, int n,
                        float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream);

/* Of n_cand fitted candidates per hand (rows i * n_cand + c of joint_angles, wrist_xf and info [n * n_cand,4], the outputs of a
 * fit) the one with the lowest info[.,0] among those whose status lacks UT_FIT_REFUSED; the lowest index among equals; a NaN
 * loses to any number.  Its 22 angles, its wrist (row 3 = (0, 0, 0, 1) when out_xf_stride >= 16),
 * its info row and its index go to row i of the outputs.  When every candidate is refused: candidate 0 with its info, index -1.
 * out_info [n,4] and out_index [n] may be NULL.  Stream ordered, no allocation, no status word: capturable.
 * UT_E_INVALID: a null required pointer, n < 0, n_cand < 1, a stride below 22 / 12. */
int ut_select_pose(const float* joint_angles, int ja_stride, const float* wrist_xf, int xf_stride, const float* info,
                   int n, int n_cand, float* out_angles, int out_ja_stride, float* out_wrist_xf, int out_xf_stride,
                   float* out_info, int32_t* out_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif
