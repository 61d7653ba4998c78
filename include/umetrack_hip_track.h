/* Sequences of 2-D detections followed frame by frame in one launch: an entry of libumetrack_hip.so in an extension header next to
 * umetrack_hip.h, like umetrack_hip_start.h and umetrack_hip_smooth.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  The conventions are those of the other headers - plain
 * device pointers and sizes, int return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - with a prototype
 * table of its own in the binding (absolutetrack_amd/_native.py: _TRACK_PROTOTYPES, pinned to this header by
 * tests/test_track_host.py). */
#ifndef UMETRACK_HIP_TRACK_H
#define UMETRACK_HIP_TRACK_H

#include "umetrack_hip_start.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `chosen` of a frame */
#define UT_TRACK_WARM 0 /* the warm fit from the previous frame's choice (or the sequence's init) */
#define UT_TRACK_COLD 1 /* the cold row was taken: a recovery, or the first usable cold row of a sequence without an init */
#define UT_TRACK_NONE 2 /* no start yet and the cold row is refused: the row is that cold row as it is */

/* n_seq sequences of n_frames frames of detections, each followed through its frames by one wave (csrc/track_views.hip): one
 * launch, not a loop of launches and read-backs.  Frame t of sequence s is row s * n_frames + t of every per-frame array, as in
 * ut_smooth_pose_sequence, and
 *  hand_model, n_models, window, weights, cam_rows, max_views, table, n_rows, table_kind, limits, mirror, t_scale, max_iters, loss,
 *  loss_scale and the outputs joint_angles, wrist_xf (strides in floats, >= 22 / >= 12; row 3 = (0, 0, 0, 1) when xf_stride >= 16)
 *  and info [n_seq * n_frames,4]
 * mean exactly what they mean for ut_fit_pose_views_robust with n = n_seq * n_frames; n_models is 1 or n_seq * n_frames.
 *  init_angles, init_wrist_xf   [n_seq] rows with the strides given: the start of each sequence's frame 0; both or neither
 *  cold_angles, cold_wrist_xf, cold_info [.,4], cold_index   [n_seq * n_frames] rows: the outputs of the cold chain
 *              ut_start_pose_views -> fit -> ut_select_pose on the same rows, cold_index as ut_select_pose writes it (< 0: every
 *              candidate was refused); all four or none.  Without them there is no recovery.
 *  recover_ratio >= 1, recover_floor >= 0 (px), both finite
 *  lengths     [n_seq] or NULL (= n_frames): rows at or past the length get no pose, an info row of 0 and chosen = -1; a length
 *              outside [0, n_frames] refuses the sequence, which writes nothing
 *  chosen      out i32 [n_seq * n_frames]: UT_TRACK_*
 * A sequence's result is, bit for bit, this chain of the existing entries.  For t = 0 .. length - 1:
 *  with a start (the sequence's init at t = 0, the previous frame's row afterwards): the warm fit ut_fit_pose_views_robust of row
 *  (s, t) from it.  lost = its status has UT_FIT_REFUSED, or (double)info[0] > recover_ratio * (double)cold_info[0] + recover_floor.
 *  When lost, with cold arrays and cold_index >= 0, the row becomes the cold row (22 angles, the wrist, the info row), chosen =
 *  UT_TRACK_COLD; otherwise the row holds the warm fit, chosen = UT_TRACK_WARM - a refused fit has given its start back, and the next
 *  frame starts from that.
 *  without a start yet: the row is the cold row; cold_index >= 0: chosen = UT_TRACK_COLD and there is a start from now on; else
 *  chosen = UT_TRACK_NONE and the next frame still has none.
 * A sequence's bits do not depend on the batch it is in, on the frames behind its length, or on trailing unused views.  residual
 * and inlier are not outputs: ask the fit or ut_pose_information_views at the returned poses.
 * Stateless: h may be NULL.  Stream ordered, no allocation.  cam_rows of every frame inside a sequence's length is checked on the
 * device before the first fit: an entry outside [-1, n_rows) writes nothing for the whole sequence and gives UT_E_INVALID ("index
 * check: ...") - from this call with UT_CHECK_SYNC or h == NULL, from the next ut_poll_status with UT_CHECK_DEFERRED, where nothing
 * synchronises and the launch is capturable.
 * UT_E_INVALID, and nothing launched: what ut_fit_pose_views_robust lists; half-given init or cold pointers, or neither an init
 * nor cold arrays; a null info or chosen; n_frames < 1, n_seq < 0, or n_seq * n_frames not fitting an int; a recover_ratio that is
 * not finite and >= 1; a recover_floor that is not finite and >= 0.  n_seq == 0 (with valid arguments otherwise): UT_OK. */
int ut_track_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                        const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                        const float* limits,
                        const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                        const float* cold_angles, int cold_ja_stride, const float* cold_wrist_xf, int cold_xf_stride,
                        const float* cold_info, const int32_t* cold_index, double recover_ratio, double recover_floor,
                        const int32_t* lengths, const int64_t* mirror, float t_scale, int max_iters, int loss, float loss_scale,
                        int n_seq, int n_frames, float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride,
                        float* info, int32_t* chosen, void* stream);

#ifdef __cplusplus
}
#endif
#endif
