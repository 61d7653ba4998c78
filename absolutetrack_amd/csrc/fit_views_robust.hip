// The pose fit on 2-D keypoints in camera views under a robust loss: ut_fit_pose_views_robust (include/umetrack_hip_robust.h).
// fit_views.hip's kernel with ut_fit_views_dev.h's cost instantiated for Huber and Geman-McClure: the same solver, region (four
// poses per workgroup, one wave per pose, no workgroup barrier), refusals and +inf rules; the weight psi multiplies into the sums
// finish_rows forms anyway, the cost hook returns the robust cost, and report also writes psi of every used observation at the
// returned pose (`inlier`), so that a caller reads the outlier classification from the launch that fitted the pose.  The yardstick
// is the float64 restatement in tests/robust_cases.py.
//
// FITV_LOSS_SQUARED without `inlier` is launch_fit_pose_views itself.  With `inlier` it is the squared instantiation of the same
// cost here, whose report writes 1 at every used observation of a pose that was not refused: the refusal is known only inside
// the fit.  Registers: DESIGN.md, "Pose from keypoints in the views, robust".
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

template <int KIND, int LOSS>
__global__ __launch_bounds__(64 * FITV_P, 2) void fit_pose_views_robust_kernel(const FitViewsRobustArgs a) {
  __shared__ FitViewsLds s_all[FITV_P];
  const FitViewsArgs& g = a.views;
  const int i = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  if (i >= g.pose.n) return;                          // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  // index check, as in fit_pose_views_kernel: a row outside [-1, n_rows) anywhere in the pose and the pose writes nothing
  bool bad_row = false;
  for (int v = 0; v < g.max_views; ++v) {
    const int r = g.cam_rows[(size_t)i * g.max_views + v];
    bad_row |= r < -1 || r >= g.n_rows;
  }
  if (bad_row) {
    if (lane == 0) atomicOr(g.status, UT_BAD_SRC_INDEX);
    return;
  }
  FitViewsCost<KIND, LOSS> cost{g};
  cost.c2 = (double)a.loss_scale * (double)a.loss_scale;
  cost.inv_c2 = 1.0 / cost.c2;
  cost.inlier = a.inlier;
  fit_pose(cost, s_all[threadIdx.x >> 6], g.pose, i, lane);
}

template <int KIND>
void launch_kind(const FitViewsRobustArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  if (a.loss == FITV_LOSS_HUBER) hipLaunchKernelGGL((fit_pose_views_robust_kernel<KIND, FITV_LOSS_HUBER>), grid, block, 0, s, a);
  else if (a.loss == FITV_LOSS_GEMAN_MCCLURE)
    hipLaunchKernelGGL((fit_pose_views_robust_kernel<KIND, FITV_LOSS_GEMAN_MCCLURE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((fit_pose_views_robust_kernel<KIND, FITV_LOSS_SQUARED>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_fit_pose_views_robust(const FitViewsRobustArgs& a, hipStream_t s) {
  if (a.loss == FITV_LOSS_SQUARED && !a.inlier) return launch_fit_pose_views(a.views, s);
  if (a.views.pose.n <= 0) return hipSuccess;
  if (a.views.max_views < 1 || a.views.max_views > TRI_MAX_VIEWS || a.loss < FITV_LOSS_SQUARED || a.loss > FITV_LOSS_GEMAN_MCCLURE)
    return hipErrorInvalidValue;
  const dim3 grid((a.views.pose.n + FITV_P - 1) / FITV_P), block(64 * FITV_P);
  if (a.views.kind == PROJECT_FISHEYE62) launch_kind<PROJECT_FISHEYE62>(a, grid, block, s);
  else launch_kind<PROJECT_PINHOLE>(a, grid, block, s);
  return hipGetLastError();
}

}  // namespace ut
