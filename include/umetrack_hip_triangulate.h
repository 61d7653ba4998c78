/* Triangulation entry of libumetrack_hip.so: an extension header next to umetrack_hip.h, like umetrack_hip_fit.h.
 *
 * umetrack_hip.h is the core boundary and its list of entries is closed; umetrack_hip_fit.h holds ut_fit_pose.  This header
 * holds the entry added after that, with the same conventions - plain device pointers and sizes, int return codes of
 * umetrack_hip.h, ut_last_error for the text, stream ordered - and a prototype table of its own in the binding
 * (absolutetrack_amd/_native.py: _TRIANGULATE_PROTOTYPES, pinned to this header by tests/test_triangulate_host.py). */
#ifndef UMETRACK_HIP_TRIANGULATE_H
#define UMETRACK_HIP_TRIANGULATE_H

#include "umetrack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The inverse of ut_project_points: the world point whose projections into several cameras meet given window coordinates,
 * for every (pose, point) of a batch in one launch.  The reference has no counterpart (its window_to_eye is a radial-only
 * fixed point that ignores p1 / p2 and serves here as the start only).  fp64 throughout (csrc/triangulate.hip;
 * tests/triangulate_cases.py is its float64 numpy restatement).
 *  window      f64 [n,max_views,n_points,2] px: the layout ut_project_points writes
 *  weights     f32 [n,max_views,n_points], each >= 0, or NULL = all 1.  The window of a weight-0 entry is never read into
 *              arithmetic: a NaN there changes nothing.  The weight of a view whose cam_rows entry is -1 is not read
 *  cam_rows, table, n_rows, table_kind   as for ut_project_points: i32 [n,max_views] rows of `table`, -1 = unused view;
 *              UT_CAMERA_FISHEYE62 rows of 32 doubles or UT_CAMERA_PINHOLE crop-camera rows of 24 doubles
 *  max_views   1..UT_TRI_MAX_VIEWS
 *  max_iters   1..64 iterations (one solve and one trial each) per point
 *  points      out f64 [n,n_points,3], or NULL
 *  points_f32  out, row i starts point_stride floats (>= 3 n_points) after row i - 1 and begins with its points: a packed
 *              [n,n_points,3] array, the keypoints inside records written in place, or the `targets` of ut_fit_pose; or NULL.
 *              The f64 result rounded once.  At least one of points and points_f32 must be given
 *  info        out f32 [n,n_points,4] or NULL: weighted rms reprojection residual sqrt(sum w r^2 / sum w) in px; sigma (below);
 *              the number of views used; status
 *  residual    out f32 [n,max_views,n_points] or NULL: the reprojection distance in px of every used view, 0 for the others -
 *              a caller rejects an outlier view from this and calls again with its weight set to 0
 * Per (pose, point):
 *  1. A view is used when its cam_rows entry is >= 0, its weight is finite and > 0, its window is finite and its start ray
 *     is finite.  A negative or non-finite weight, a non-finite window at a positive weight, or fewer than 2 used views:
 *     UT_TRI_REFUSED.
 *  2. Start: the weighted least-squares intersection of the used views' rays, sum w (I - d d^T) X = sum w (I - d d^T) o, by
 *     a 3 x 3 Cholesky factorisation.  Fisheye62 rays come from the reference's own unprojection (Fisheye62CameraModel
 *     .window_to_eye, lib/common/camera.py:146-181), pinhole rays from ((x - c) / f, 1), both rotated to the world.  A pivot at
 *     or below UT_TRI_PIVOT_FRACTION of the largest diagonal entry means parallel rays - two views of one and the same camera
 *     are the simplest case: UT_TRI_DEGENERATE.  So does an intersection that cannot be projected into every used view (a
 *     non-finite window, or behind the near plane of a pinhole view).
 *  3. Levenberg-Marquardt on sum_v w_v |project_v(X) - window_v|^2 through the exact forward model of ut_project_points, with
 *     the analytic 2 x 3 Jacobian per view; the damped matrix is H + lambda diag(H).  A trial is accepted only when the cost
 *     goes down; lambda starts at UT_TRI_LAMBDA_START, x 0.1 on acceptance (not below UT_TRI_LAMBDA_MIN), x 10 on rejection.
 *     A trial that is not finite, that lies in front of the near plane (eye z < UT_TRI_NEAR_Z) of a used pinhole view, or
 *     whose factorisation meets a non-positive pivot is a rejected step, never a NaN in the output.  The point stops with
 *     UT_TRI_CONVERGED when a valid trial's step is at most UT_TRI_STEP_TOL sqrt(1 + |X|^2) under a lambda of at most
 *     UT_TRI_LAMBDA_CONVERGED_MAX (accepted or not), or when a rejected valid trial's rms residual is within
 *     UT_TRI_FLAT_TOL_PX of the accepted one (noisy windows: the cost cannot resolve a smaller step); otherwise at max_iters
 *     with UT_TRI_AT_MAX_ITERS and the best point found.
 *  4. sigma = sqrt(trace((sum_v w_v J_v^T J_v)^-1)) at the solution: model units per pixel of detection noise when the weights
 *     are 1 - to first order, noise_px * sigma is the rms distance by which isotropic noise of noise_px on every window moves
 *     the point.  +inf when that matrix cannot be factorised.
 * Refused and degenerate points: point (0, 0, 0), sigma +inf, rms 0, views = the number of used views, residuals 0.
 * Views are summed in ascending order and a point's result does not depend on the batch it is in.  Stateless: h may be
 * NULL.  Stream ordered, no allocation.  cam_rows is checked on the device: an entry outside [-1, n_rows) writes nothing for
 * its pose and gives UT_E_INVALID ("index check: ...") - from this call with UT_CHECK_SYNC or h == NULL, from the next
 * ut_poll_status with UT_CHECK_DEFERRED, where nothing synchronises and the launch is capturable.
 * UT_E_INVALID, and nothing launched: a null window / cam_rows / table, both point outputs null, point_stride < 3 n_points
 * with points_f32 given, max_views outside 1..UT_TRI_MAX_VIEWS, max_iters outside 1..64, n_points < 1, n_rows < 1, n < 0, an
 * unknown table_kind, a handle of another device than the one `window` lives on.  n == 0 (with valid arguments otherwise):
 * UT_OK, nothing launched. */
enum { UT_TRI_CONVERGED = 1, UT_TRI_AT_MAX_ITERS = 2, UT_TRI_REFUSED = 4, UT_TRI_DEGENERATE = 8 };
#define UT_TRI_MAX_VIEWS 8
#define UT_TRI_PIVOT_FRACTION 1e-10
#define UT_TRI_LAMBDA_START 1e-6
#define UT_TRI_LAMBDA_MIN 1e-12
#define UT_TRI_LAMBDA_CONVERGED_MAX 1.0
#define UT_TRI_STEP_TOL 1e-12
#define UT_TRI_FLAT_TOL_PX 1e-11
#define UT_TRI_NEAR_Z 1e-4
int ut_triangulate_points(ut_handle h, const double* window, const float* weights, const int32_t* cam_rows, int max_views,
                          const double* table, int n_rows, int table_kind, int n_points, int n, int max_iters,
                          double* points, float* points_f32, int point_stride, float* info, float* residual, void* stream);

#ifdef __cplusplus
}
#endif
#endif
