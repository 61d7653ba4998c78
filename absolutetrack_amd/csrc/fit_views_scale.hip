// The pose fit on 2-D keypoints in camera views with the hand's scale as a 27th parameter: ut_fit_pose_views_scale
// (include/umetrack_hip_views_scale.h).  It is to ut_fit_pose_views_robust what fit_scale.hip is to fit.hip: the solver is
// ut_fit_dev.h's fit_pose(), the cost is ut_fit_views_dev.h's FitViewsCost - every loss - on 27 parameters, sigma = ln s ordered
// last, and the scale's column, trial, bounds and information are fit_scale.hip's.  The yardstick is the float64 restatement in
// tests/views_scale_cases.py.
//
// Scale s means hand.scaled_hand_model(model, s).  d landmark / d sigma = landmark - wrist translation goes into column 26 of
// the landmark's three rows BEFORE the views' L^T transform, which then runs over all 27 columns: the 63 rows' J^T J and J^T r
// are the normal equations of the stacked reprojection residuals whose sigma column is J_v (p - t) per view.  In fixed mode the
// column stays zero, the floored diagonal gives d sigma = 0 and the scale is kept by construction as well.  Every trial writes
// the region's model again from the unscaled rest coordinates at clamp(s exp(d sigma)), and a small step also needs
// |d sigma| <= FIT_STEP_TOL.  After the loop the scale information of the accepted state, the last pivot of the factorisation
// of A + SCALE_INFO_LAMBDA D, as in fit_scale.hip; then, for `residual` and `inlier`, the region's model is put back to the
// accepted scale (a rejected last trial left its own there) before the returned pose is evaluated once more.
//
// One camera cannot see the hand's size: scaling the world about a central camera leaves every projection unchanged, so a free
// fit on one view converges to a scale that means nothing and says so through an information some four orders of magnitude
// below a two-view fit's.  UT_SCALE_FIXED is what one-view frames are for.
//
// The region is fit_scale.hip's (16416 bytes, row stride 29): three poses per workgroup, one wave per pose, 49248 bytes of
// static LDS.  Registers and times: DESIGN.md, "Hand scale from keypoints in the views".
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

constexpr int FITVS_P = 3;        // poses (waves) per workgroup
constexpr int FITVS_SIGMA = 26;   // column of sigma = ln s

struct FitViewsScaleLds {         // one wave's region: fit_scale.hip's members
  float hm[321];                  // the pose's packed model at the scale of the last evaluated state
  float rest[129];                // its joint (66) and landmark (63) rest coordinates as given: hm[66..194] = rest * scale
  float local[20][12];            // joint transforms of the last evaluated state
  float prefix[20][12];           // W L0 .. L(j-1) in front of joint 4 f + j
  float frame[17][12];            // skinning frames
  float omega[20][3], cw[20][3];  // joint axes and centres in the world (linearisation)
  float jl[63 * 29];              // J while the normal matrix is formed, then the Cholesky factor L [27][29]
  float a[28][29];                // lower triangle of [J r]^T [J r]: A = J^T J, row 27 = g = J^T r
  float ang[20], ang_t[20];       // accepted and trial angles
  float wrist[12], wrist_t[12];   // accepted and trial wrist frame
  float p[21][3];                 // landmarks of the last evaluated state
  float target[21][3], w[21];     // 0 (no 3-D targets) and scalar weights sum_v w_vl, 0 = unused
};
static_assert(sizeof(FitViewsScaleLds) == 16416 && sizeof(FitViewsScaleLds) * FITVS_P <= 65536, "a workgroup's static LDS");

template <int KIND, int LOSS>
struct FitViewsScaleCost : FitViewsCost<KIND, LOSS, FitViewsScaleLds, 27, 29> {
  using Views = FitViewsCost<KIND, LOSS, FitViewsScaleLds, 27, 29>;
  using Lds = FitViewsScaleLds;
  static constexpr int NP = Views::NP, LD = Views::LD;
  const FitViewsScaleArgs& g;
  bool fixed = false;
  float scale = 1.f, scale_t = 1.f;      // of the accepted and of the trial state

  __device__ inline explicit FitViewsScaleCost(const FitViewsScaleArgs& args) : Views{args.robust.views}, g(args) {}

  // The model of the region at scale s: the bits of scaled_hand_model.  Called by the whole wave; the caller syncs.
  __device__ inline void set_scale(Lds& S, float s, int lane) {
    for (int e = lane; e < 129; e += 64) S.hm[66 + e] = S.rest[e] * s;
  }

  // The unscaled rest coordinates and the start's scale, which must lie inside the bounds; the model at that scale; then the
  // observations.
  __device__ inline bool load(Lds& S, int i, int mrow, int lane, float& wl, bool& used) {
    fixed = g.scale_mode == FITS_MODE_FIXED;
    for (int e = lane; e < 129; e += 64) S.rest[e] = this->a.pose.hand_model[(size_t)mrow * 321 + 66 + e];
    if (g.init_scale) scale = g.init_scale[i];
    const bool bad_scale = !(scale >= FITS_SCALE_MIN) || !(scale <= FITS_SCALE_MAX);      // a NaN is neither
    if (bad_scale) scale = 1.f;
    wave_sync();                                      // S.hm is written by other lanes
    set_scale(S, scale, lane);
    return Views::load(S, i, mrow, lane, wl, used) && !bad_scale;
  }
  // d landmark / d ln s in front of the residual column, left zero when the scale is fixed; then the views' whitening of all
  // 27 columns
  __device__ inline void finish_rows(Lds& S, int lane, float* row, float sw, float px, float py, float pz) {
    if (!fixed) {
      row[FITVS_SIGMA] = px - S.wrist[3];
      row[LD + FITVS_SIGMA] = py - S.wrist[7];
      row[2 * LD + FITVS_SIGMA] = pz - S.wrist[11];
    }
    Views::finish_rows(S, lane, row, sw, px, py, pz);
  }
  __device__ inline bool trial(Lds& S, int lane, float delta) {
    const float ds = fixed ? 0.f : lane_value(delta, FITVS_SIGMA);
    scale_t = fixed ? scale : fminf(fmaxf(scale * expf(ds), FITS_SCALE_MIN), FITS_SCALE_MAX);
    set_scale(S, scale_t, lane);
    return fabsf(ds) <= FIT_STEP_TOL;
  }
  __device__ inline void keep() { Views::keep(); scale = scale_t; }

  // scale (1 for a refused pose); info [n,6]: the views' four columns, the scale information, 0; residual and inlier
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    int status = st.status;
    float scale_info = 0.f;
    if (!st.refused && !fixed) {
      // the scale information at the accepted state, as in fit_scale.hip: after an accepted last trial the region holds that
      // state and the normal matrix is the one before it; after a rejected one the normal matrix is the accepted state's
      if (st.fresh) fit_linearise(*this, S, lane, st);
      float pivot = 0.f;                              // stays 0 when a pivot is not positive and finite
      fit_solve<NP, LD, false>(S, lane, FITS_SCALE_INFO_LAMBDA, fit_diag<NP>(S, lane), pivot);
      scale_info = uniform(pivot);
      if (scale <= FITS_SCALE_MIN || scale >= FITS_SCALE_MAX) status |= FITS_AT_BOUND;
    }
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
__global__ __launch_bounds__(64 * FITVS_P, 2) void fit_pose_views_scale_kernel(const FitViewsScaleArgs a) {
  __shared__ FitViewsScaleLds s_all[FITVS_P];
  const FitViewsArgs& g = a.robust.views;
  const int i = blockIdx.x * FITVS_P + (threadIdx.x >> 6);
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
  const dim3 grid((g.pose.n + FITVS_P - 1) / FITVS_P), block(64 * FITVS_P);
  if (g.kind == PROJECT_FISHEYE62) launch_kind<PROJECT_FISHEYE62>(a, grid, block, s);
  else launch_kind<PROJECT_PINHOLE>(a, grid, block, s);
  return hipGetLastError();
}

}  // namespace ut
