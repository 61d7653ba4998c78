// The pose fit on 2-D keypoints in camera views with the hand's scale as a 27th parameter: ut_fit_pose_views_scale
// (include/umetrack_hip_views_scale.h).  It is to ut_fit_pose_views_robust what fit_scale.hip is to fit.hip: the solver is
// ut_fit_dev.h's fit_pose(), the cost is ut_fit_views_dev.h's FitViewsCost - every loss - on 27 parameters, sigma = ln s ordered
// last, and the scale's region, start, trial, bounds and information are ut_fit_dev.h's FitScaleParam, the base this problem
// shares with fit_scale.hip's.  The yardstick is the float64 restatement in tests/views_scale_cases.py.
//
// d landmark / d sigma = landmark - wrist translation goes into column 26 of the landmark's three rows BEFORE the views' L^T
// transform, which then runs over all 27 columns: the 63 rows' J^T J and J^T r are the normal equations of the stacked
// reprojection residuals whose sigma column is J_v (p - t) per view.  In fixed mode the column stays zero, the floored diagonal
// gives d sigma = 0 and the scale is kept by construction as well.  After the loop the scale information of the accepted state
// (FitScaleParam::scale_information); then, for `residual` and `inlier`, the region's model is put back to the accepted scale
// (a rejected last trial left its own there) before the returned pose is evaluated once more.
//
// One camera cannot see the hand's size: scaling the world about a central camera leaves every projection unchanged, so a free
// fit on one view converges to a scale that means nothing and says so through an information some four orders of magnitude
// below a two-view fit's.  UT_SCALE_FIXED is what one-view frames are for.
//
// The region is FitScaleLds (16416 bytes, row stride 29): FITS_P = three poses per workgroup, one wave per pose, 49248 bytes of
// static LDS.  Registers and times: DESIGN.md, "Hand scale from keypoints in the views".
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

template <int KIND, int LOSS>
struct FitViewsScaleCost : FitViewsCost<KIND, LOSS, FitScaleLds, 27, 29>, FitScaleParam {
  using Views = FitViewsCost<KIND, LOSS, FitScaleLds, 27, 29>;
  using Lds = FitScaleLds;
  static constexpr int NP = Views::NP, LD = Views::LD;
  const FitViewsScaleArgs& g;

  __device__ inline explicit FitViewsScaleCost(const FitViewsScaleArgs& args) : Views{args.robust.views}, g(args) {}

  // the scale's start, then the observations
  __device__ inline bool load(Lds& S, int i, int mrow, int lane, float& wl, bool& used) {
    const bool ok = load_scale(S, this->a.pose.hand_model, mrow, g.init_scale, g.scale_mode, i, lane);
    return Views::load(S, i, mrow, lane, wl, used) && ok;
  }
  // d landmark / d ln s in front of the residual column, left zero when the scale is fixed; then the views' whitening of all
  // 27 columns
  __device__ inline void finish_rows(Lds& S, int lane, float* row, float sw, float px, float py, float pz) {
    if (!fixed) {
      row[FITS_SIGMA] = px - S.wrist[3];
      row[LD + FITS_SIGMA] = py - S.wrist[7];
      row[2 * LD + FITS_SIGMA] = pz - S.wrist[11];
    }
    Views::finish_rows(S, lane, row, sw, px, py, pz);
  }
  __device__ inline bool trial(Lds& S, int lane, float delta) { return FitScaleParam::trial(S, lane, delta); }
  __device__ inline void keep() { Views::keep(); scale = scale_t; }

  // scale (1 for a refused pose); info [n,6]: the views' four columns, the scale information, 0; residual and inlier
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    int status = st.status;
    const float scale_info = scale_information(*this, S, lane, st, status);
    if (lane == 0) g.scale[i] = st.refused ? 1.f : scale;
    if (this->a.info && lane == 0) {
      float* o = this->a.info + (size_t)i * 6;
      FitState s = st;
      s.worst = this->worst;
      fit_store_info(o, s, st.wsum, status);
      o[4] = scale_info;
      o[5] = 0.f;
    }
    if (!st.refused && (this->a.residual || this->inlier)) {
      wave_sync();                                    // a rejected last trial left its own scale in the region's model
      set_scale(S, scale, lane);
      wave_sync();
    }
    Views::report_observations(S, i, lane, st);
  }
};

template <int KIND, int LOSS>
__global__ __launch_bounds__(64 * FITS_P, 2) void fit_pose_views_scale_kernel(const FitViewsScaleArgs a) {
  __shared__ FitScaleLds s_all[FITS_P];
  const FitViewsArgs& g = a.robust.views;
  const int i = blockIdx.x * FITS_P + (threadIdx.x >> 6);
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
  FitViewsScaleCost<KIND, LOSS> cost(a);
  cost.c2 = (double)a.robust.loss_scale * (double)a.robust.loss_scale;
  cost.inv_c2 = 1.0 / cost.c2;
  cost.inlier = a.robust.inlier;
  fit_pose(cost, s_all[threadIdx.x >> 6], g.pose, i, lane);
}

template <int KIND>
void launch_kind(const FitViewsScaleArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  if (a.robust.loss == FITV_LOSS_HUBER) hipLaunchKernelGGL((fit_pose_views_scale_kernel<KIND, FITV_LOSS_HUBER>), grid, block, 0, s, a);
  else if (a.robust.loss == FITV_LOSS_GEMAN_MCCLURE)
    hipLaunchKernelGGL((fit_pose_views_scale_kernel<KIND, FITV_LOSS_GEMAN_MCCLURE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((fit_pose_views_scale_kernel<KIND, FITV_LOSS_SQUARED>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_fit_pose_views_scale(const FitViewsScaleArgs& a, hipStream_t s) {
  const FitViewsArgs& g = a.robust.views;
  if (g.pose.n <= 0) return hipSuccess;
  if (g.max_views < 1 || g.max_views > TRI_MAX_VIEWS || a.robust.loss < FITV_LOSS_SQUARED || a.robust.loss > FITV_LOSS_GEMAN_MCCLURE ||
      (a.scale_mode != FITS_MODE_FREE && a.scale_mode != FITS_MODE_FIXED) || !a.scale)
    return hipErrorInvalidValue;
  const dim3 grid((g.pose.n + FITS_P - 1) / FITS_P), block(64 * FITS_P);
  if (g.kind == PROJECT_FISHEYE62) launch_kind<PROJECT_FISHEYE62>(a, grid, block, s);
  else launch_kind<PROJECT_PINHOLE>(a, grid, block, s);
  return hipGetLastError();
}

}  // namespace ut
