/* Keypoints with their information, entries of libumetrack_hip.so: an extension header next to umetrack_hip.h, like
 * umetrack_hip_fit.h, umetrack_hip_triangulate.h and umetrack_hip_scale.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed.  This header holds the two entries that carry a
 * landmark's 3 x 3 information from the triangulation into the pose fit, with the conventions of the other headers - plain
 * device pointers and sizes, int return codes of umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype
 * table of its own in the binding (absolutetrack_amd/_native.py: _INFO_PROTOTYPES, pinned to this header by
 * tests/test_info_host.py). */
#ifndef UMETRACK_HIP_INFO_H
#define UMETRACK_HIP_INFO_H

#include "umetrack_hip_fit.h"
#include "umetrack_hip_triangulate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The factor of a landmark's information: six floats (l00, l10, l11, l20, l21, l22), the lower Cholesky factor L of a
 * symmetric 3 x 3 matrix H = L L^T.  To first order, moving the landmark by d costs |L^T d|^2. */
#define UT_INFO_FACTOR_FLOATS 6

/* ut_triangulate_points (umetrack_hip_triangulate.h) that also hands out what it knows about each point.  Every argument and
 * every other output as there, bit for bit; in addition
 *  sqrt_info   out f32 [n,n_points,6], required: the factor of H = sum_v w_v J_v^T J_v at the returned point - the
 *              factorisation step 4 performs for sigma, so sigma = sqrt(trace((L L^T)^-1)) -, computed in fp64 and rounded once.
 *              In px per model unit when the weights are 1: |L^T d|^2 is the reprojection cost of moving the point by d.  All
 *              six entries are 0 for refused and degenerate points and wherever sigma is +inf; a pose whose cam_rows fail the
 *              index check writes nothing here either.
 * UT_E_INVALID, and nothing launched: as for ut_triangulate_points, and a null sqrt_info. */
int ut_triangulate_points_info(ut_handle h, const double* window, const float* weights, const int32_t* cam_rows, int max_views,
                               const double* table, int n_rows, int table_kind, int n_points, int n, int max_iters,
                               double* points, float* points_f32, int point_stride, float* info, float* residual,
                               float* sqrt_info, void* stream);

/* ut_fit_pose (umetrack_hip_fit.h) on landmarks that come with their information: the pose whose landmarks minimise
 * sum_l |L_l^T (landmark_l - target_l)|^2 (csrc/fit_info.hip; tests/info_cases.py is its float64 restatement).  With the
 * factors of ut_triangulate_points_info this is one Gauss-Newton linearisation of the views' reprojection cost about the
 * triangulated points: depth, which a narrow baseline measures badly, counts for little, and the hand's known size fixes it
 * instead.  Factors from anywhere else - a depth sensor's or a motion capture system's covariances - serve as well:
 * L = chol(covariance^-1).  Every argument as for ut_fit_pose, with
 *  sqrt_info   f32 [n,21,6], required, in place of `weights`.  A landmark is used when any entry of its factor is non-zero;
 *              the target of an unused landmark is never read into arithmetic: a NaN there changes nothing.  The scalar weight
 *              of a landmark - for the centroid the wrist increment turns about, the extent that scales the translation's
 *              step tolerance and the cold start's Kabsch fit - is its factor's squared Frobenius norm, trace(H).  Factors
 *              sqrt(w) I give the cost of ut_fit_pose with weights w
 *  info        [n,4] or NULL: sqrt(cost / (3 x used landmarks)), the whitened rms - px when the factors come from the
 *              triangulation -; the largest Euclidean residual of a used landmark, in target units; iterations run; status
 * Solver, constants, stop rules, status bits (UT_FIT_*), outputs and their in-place use: ut_fit_pose's.  UT_FIT_REFUSED: a factor
 * entry that is not finite, a non-finite target of a used landmark, fewer than 3 used landmarks; outputs then as for
 * ut_fit_pose.
 * Start.  Both init pointers NULL: ut_fit_pose's cold start, the rest pose aligned by a Kabsch fit weighted with trace(H).  It
 * is kept for symmetry with ut_fit_pose and is NOT the recommended start: the anisotropic cost has flat directions along the
 * viewing rays, and a cold start can end in a local minimum (1 of the 74 hands of tests/triangulate_cases.py golden_case does,
 * worst landmark 35 mm, on exact targets).  Run ut_fit_pose on the used landmarks first (weights 1 / 0) and pass its outputs
 * as the init - two launches with no host work between them, which is what the Python layers do.
 * A pose's result does not depend on the batch it is in.  Stateless: h may be NULL.  Stream ordered, no allocation, no
 * synchronisation: capturable.  UT_E_INVALID, and nothing launched: as for ut_fit_pose, and a null sqrt_info. */
int ut_fit_pose_info(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                     const float* sqrt_info, const float* limits, const float* init_angles, int init_ja_stride,
                     const float* init_wrist_xf, int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int n,
                     float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
