// The pose fit with the hand's scale as a 27th parameter, fp32, and the pool that turns per-pose scales into one:
// ut_fit_pose_scale and ut_pool_scale (include/umetrack_hip_scale.h).  The reference calibrates a hand's scale only through
// its network (run_eval_unknown_skeleton.py:55-76); the yardstick is the float64 restatement in tests/scale_cases.py.
//
// The scale parameter itself - the region, sigma = ln s ordered last, the trial scale and its bounds, the scale information of
// the accepted state - is ut_fit_dev.h's FitScaleParam, shared with fit_views_scale.hip.  The solver is ut_fit_dev.h's fit_pose()
// and the cost is fit.hip's, on 27 parameters.  Every trial evaluates ut_fk's arithmetic (ut_fk.h) on the region's model at the
// trial scale: ut_fk on the blob of scaled_hand_model(model, s) with the output pose reproduces the residual the solver saw.
//
// A region is 16416 bytes (row stride 29: odd, like fit.hip's 27), so three poses share the 64 KB of static LDS a workgroup
// gets; a fourth would need 65664.
#include "ut_fit_dev.h"

namespace ut {
namespace {

struct FitScaleCost : FitScaleParam {
  using Lds = FitScaleLds;
  static constexpr int NP = 27, LD = 29;
  const FitScaleArgs& a;

  __device__ inline explicit FitScaleCost(const FitScaleArgs& args) : a(args) {}

  __device__ inline bool load(Lds& S, int i, int mrow, int lane, float& wl, bool& used) {
    const bool ok = load_scale(S, a.pose.hand_model, mrow, a.init_scale, a.scale_mode, i, lane);
    return fit_scalar_weight(a.weights, i, lane, wl, used) && ok;
  }
  __device__ inline float row_scale(const Lds& S, int lane) { return sqrtf(S.w[lane]); }
  // d landmark / d ln s in front of the residual column; left zero when the scale is fixed
  __device__ inline void finish_rows(Lds& S, int, float* row, float sw, float px, float py, float pz) {
    if (fixed) return;
    row[FITS_SIGMA] = sw * (px - S.wrist[3]);
    row[LD + FITS_SIGMA] = sw * (py - S.wrist[7]);
    row[2 * LD + FITS_SIGMA] = sw * (pz - S.wrist[11]);
  }
  __device__ inline float cost(const Lds&, int, bool, float isotropic) { return isotropic; }
  __device__ inline void keep() { scale = scale_t; }
  // A refused pose has scale 1.
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    int status = st.status;
    const float scale_info = scale_information(*this, S, lane, st, status);
    if (lane == 0) a.scale[i] = st.refused ? 1.f : scale;
    if (a.info && lane == 0) {
      float* o = a.info + (size_t)i * 6;
      fit_store_info(o, st, st.wsum, status);
      o[4] = scale_info;
      o[5] = 0.f;
    }
  }
};

__global__ __launch_bounds__(64 * FITS_P) void fit_pose_scale_kernel(const FitScaleArgs a) {
  __shared__ FitScaleLds s_all[FITS_P];
  const int i = blockIdx.x * FITS_P + (threadIdx.x >> 6);
  if (i >= a.pose.n) return;                          // whole waves leave; nobody waits for them
  FitScaleCost cost{a};
  fit_pose(cost, s_all[threadIdx.x >> 6], a.pose, i, threadIdx.x & 63);
}

// One wave per group of group_size consecutive poses: the information-weighted mean of ln s in fp64.  Lanes stride over the
// group in a fixed order and the sums go through the butterfly, so a group's row depends on its own poses alone.
__global__ __launch_bounds__(64) void pool_scale_kernel(const float* __restrict__ scale, const float* __restrict__ info,
                                                        int group_size, float* __restrict__ group,
                                                        float* __restrict__ pose_scale) {
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * group_size;
  double si = 0.0, sil = 0.0, cnt = 0.0;
  for (int k = lane; k < group_size; k += 64) {
    const float* o = info + (base + k) * 6;
    const int status = (int)o[3];
    const float inf = o[4];
    const bool use = (status & FITS_CONVERGED) && !(status & (FITS_REFUSED | FITS_AT_BOUND)) && inf > 0.f && inf <= 3.0e38f;
    if (use) {
      const double l = log((double)scale[base + k]);
      si += (double)inf; sil += (double)inf * l; cnt += 1.0;
    }
  }
  si = wave_sum(si); sil = wave_sum(sil); cnt = wave_sum(cnt);
  const bool any = cnt > 0.0;
  const double mean = any ? sil / si : 0.0;
  double ss = 0.0;
  for (int k = lane; k < group_size; k += 64) {
    const float* o = info + (base + k) * 6;
    const int status = (int)o[3];
    const float inf = o[4];
    const bool use = (status & FITS_CONVERGED) && !(status & (FITS_REFUSED | FITS_AT_BOUND)) && inf > 0.f && inf <= 3.0e38f;
    if (use) {
      const double dl = log((double)scale[base + k]) - mean;
      ss += (double)inf * dl * dl;
    }
  }
  ss = wave_sum(ss);
  const float pooled = any ? (float)exp(mean) : 1.f;
  if (lane == 0) {
    float* g = group + (size_t)blockIdx.x * 4;
    g[0] = pooled;
    g[1] = any ? (float)(1.0 / sqrt(si)) : __int_as_float(0x7f800000);
    g[2] = any ? (float)sqrt(ss / fmax(cnt - 1.0, 1.0)) : 0.f;
    g[3] = (float)cnt;
  }
  if (pose_scale)
    for (int k = lane; k < group_size; k += 64) pose_scale[base + k] = pooled;
}

}  // namespace

hipError_t launch_fit_pose_scale(const FitScaleArgs& a, hipStream_t s) {
  if (a.pose.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fit_pose_scale_kernel, dim3((a.pose.n + FITS_P - 1) / FITS_P), dim3(64 * FITS_P), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_scale(const float* scale, const float* info, int n_groups, int group_size, float* group,
                             float* pose_scale, hipStream_t s) {
  if (n_groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(pool_scale_kernel, dim3(n_groups), dim3(64), 0, s, scale, info, group_size, group, pose_scale);
  return hipGetLastError();
}

}  // namespace ut
