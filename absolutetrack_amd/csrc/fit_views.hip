// The pose fit on 2-D keypoints in camera views, fp32 solver with an fp64 projection: ut_fit_pose_views
// (include/umetrack_hip_views.h).  The cost is the reprojection error itself, sum_v sum_l w_vl |project_v(landmark_l) - u_vl|^2,
// over every detection of every view through the exact camera model of ut_project_points / ut_triangulate_points - a landmark
// that one camera alone sees counts, and a hand that one camera alone sees can be fitted: its known size fixes its depth.  The
// yardstick is the float64 restatement in tests/views_cases.py.
//
// This is ut_fit_pose_info (fit_info.hip) with the factor derived again at every accepted state and the virtual target moved
// with it.  The solver is ut_fit_dev.h's fit_pose(), on fit.hip's 26 parameters and 63 rows.  At each linearisation the lane of
// landmark l computes, in fp64 with the views in ascending order, M = sum_v w_v J_v^T J_v (3 x 3, positive semidefinite) and
// b = sum_v w_v J_v^T r_v with the analytic 2 x 3 Jacobian J_v of ut_camera.h's project_jac, factors M = L L^T by the
// semidefinite Cholesky of ut_camera.h (a pivot at or below UT_TRI_PIVOT_FRACTION x the largest diagonal entry zeroes its column:
// one view gives rank 2), solves L rho = b, and replaces its three Jacobian rows a by L^T a - as fit_info.hip's finish_rows
// does - and its residual column by rho.  J^T J and J^T r of the 63 rows are then the Gauss-Newton normal equations of the
// stacked 2 x views x 21 reprojection residuals, which would not fit a region.  The cost hook evaluates the true reprojection
// cost of the state fit_eval left in S.p: per landmark in fp64 over ascending views, rounded once, then wave_sum.  A state in
// which a used observation is not finite or lies in front of UT_TRI_NEAR_Z of a used pinhole view costs +inf: a rejected trial,
// or a refused start.  There are no 3-D targets: the wrist increment turns about the weighted centroid of the START's
// landmarks (weight sum_v w_vl), whose extent scales the translation's step tolerance (PIVOT_FROM_START of ut_fit_dev.h).
//
// Windows, weights and camera rows stay in global memory: a lane reads each of its values once per evaluation, a pose's 21
// lanes share its camera rows, and a launch's rows stay in L2.  The region is FitInfoLds without the factors: 4 x 15064 =
// 60256 bytes of the 64 KB a workgroup gets.  The projection is fp64 on the fp32 landmark: project - u is the difference of
// two numbers of some 300 px, where fp32 would lose the cost's digits.  This file keeps the default contraction, like fit.hip.
//
// Registers.  With the fp64 projection inlined and nothing said, the Fisheye62 kernel takes 256 VGPRs and 5 AGPRs - one wave
// per SIMD, where fit_pose_info_kernel's 227 leave room for two workgroups per CU - and 8192 hands take 2.16 x
// ut_fit_pose_info's time.  __launch_bounds__(256, 2) holds it to 254 VGPRs without scratch: 1.44 x.  The projection out of
// line (arguments and results by value) took 193 VGPRs, 80 bytes of scratch per lane for the call frames and 1.29 x, but was
// one iteration over the iteration rule of tests/test_gpu_views.py on 2 of 148 full fits; windows and weights in LDS (three
// poses per workgroup) 1.53 x.  DESIGN.md, "Pose from keypoints in the views", has the table.
//
// The cost (FitViewsCost) and the region (FitViewsLds) live in ut_fit_views_dev.h, with the loss as a compile-time parameter that
// fit_views_robust.hip instantiates for Huber and Geman-McClure; here it is the squared loss, and this file's device code is what
// it was before the loss became a parameter (tools/compare_device_asm.py).
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

template <int KIND>
__global__ __launch_bounds__(64 * FITV_P, 2) void fit_pose_views_kernel(const FitViewsArgs a) {
  __shared__ FitViewsLds s_all[FITV_P];
  const int i = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  if (i >= a.pose.n) return;                          // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  // index check: a row outside [-1, n_rows) anywhere in the pose and the pose writes nothing
  bool bad_row = false;
  for (int v = 0; v < a.max_views; ++v) {
    const int r = a.cam_rows[(size_t)i * a.max_views + v];
    bad_row |= r < -1 || r >= a.n_rows;
  }
  if (bad_row) {
    if (lane == 0) atomicOr(a.status, UT_BAD_SRC_INDEX);
    return;
  }
  FitViewsCost<KIND> cost{a};
  fit_pose(cost, s_all[threadIdx.x >> 6], a.pose, i, lane);
}

}  // namespace

hipError_t launch_fit_pose_views(const FitViewsArgs& a, hipStream_t s) {
  if (a.pose.n <= 0) return hipSuccess;
  if (a.max_views < 1 || a.max_views > TRI_MAX_VIEWS) return hipErrorInvalidValue;
  const dim3 grid((a.pose.n + FITV_P - 1) / FITV_P), block(64 * FITV_P);
  if (a.kind == PROJECT_FISHEYE62) hipLaunchKernelGGL(fit_pose_views_kernel<PROJECT_FISHEYE62>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(fit_pose_views_kernel<PROJECT_PINHOLE>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
