// The pose fit with the hand's scale as a 27th parameter, fp32, and the pool that turns per-pose scales into one:
// ut_fit_pose_scale and ut_pool_scale (include/umetrack_hip_scale.h).  The reference calibrates a hand's scale only through
// its network (run_eval_unknown_skeleton.py:55-76); the yardstick is the float64 restatement in tests/scale_cases.py.
//
// Scale s means hand.scaled_hand_model(model, s): the 66 joint and 63 landmark rest coordinates times s in fp32, nothing
// else.  The solver is ut_fit_dev.h's fit_pose() and the cost is fit.hip's, on 27 parameters: sigma = ln s is ordered last,
// d landmark / d sigma = landmark - wrist translation (every length grows about the wrist frame's origin), the trial scale
// is clamp(s exp(d sigma), SCALE_MIN, SCALE_MAX), and a small step also needs |d sigma| <= FIT_STEP_TOL.  Every trial writes
// the pose's LDS model again from an unscaled copy of those 129 floats and evaluates ut_fk's arithmetic (ut_fk.h) on it: ut_fk
// on the blob of scaled_hand_model(model, s) with the output pose reproduces the residual the solver saw.  After the loop the
// scale information of the accepted state: the last pivot of the Cholesky factorisation of A + SCALE_INFO_LAMBDA D, i.e. the
// Schur complement of sigma.
//
// A region is 16416 bytes (row stride 29: odd, like fit.hip's 27), so three poses share the 64 KB of static LDS a workgroup
// gets; a fourth would need 65664.
#include "ut_fit_dev.h"

namespace ut {
namespace {

constexpr int FITS_P = 3;         // poses (waves) per workgroup
constexpr int FITS_SIGMA = 26;    // column of sigma = ln s

struct FitScaleLds {              // one wave's region
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
  float target[21][3], w[21];     // targets (0 where the weight is 0) and weights
};
static_assert(sizeof(FitScaleLds) == 16416 && sizeof(FitScaleLds) * FITS_P <= 65536, "a workgroup's static LDS");

struct FitScaleCost {
  using Lds = FitScaleLds;
  static constexpr int NP = 27, LD = 29;
  const FitScaleArgs& a;
  bool fixed;
  float scale = 1.f, scale_t = 1.f;      // of the accepted and of the trial state

  // The model of the region at scale s: the bits of scaled_hand_model.  Called by the whole wave; the caller syncs.
  __device__ inline void set_scale(Lds& S, float s, int lane) {
    for (int e = lane; e < 129; e += 64) S.hm[66 + e] = S.rest[e] * s;
  }

  // The unscaled rest coordinates and the start's scale, which must lie inside the bounds; the model at that scale.
  __device__ inline bool load(Lds& S, int i, int mrow, int lane, float& wl, bool& used) {
    fixed = a.scale_mode == FITS_MODE_FIXED;
    for (int e = lane; e < 129; e += 64) S.rest[e] = a.pose.hand_model[(size_t)mrow * 321 + 66 + e];
    if (a.init_scale) scale = a.init_scale[i];
    const bool bad_scale = !(scale >= FITS_SCALE_MIN) || !(scale <= FITS_SCALE_MAX);      // a NaN is neither
    if (bad_scale) scale = 1.f;
    wave_sync();                                      // S.hm is written by other lanes
    set_scale(S, scale, lane);
    return fit_scalar_weight(a.weights, i, lane, wl, used) && !bad_scale;
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
  __device__ inline bool trial(Lds& S, int lane, float delta) {
    // with the sigma column zero the floored diagonal gives d sigma = 0; the fixed scale is kept by construction as well
    const float ds = fixed ? 0.f : lane_value(delta, FITS_SIGMA);
    scale_t = fixed ? scale : fminf(fmaxf(scale * expf(ds), FITS_SCALE_MIN), FITS_SCALE_MAX);
    set_scale(S, scale_t, lane);
    return fabsf(ds) <= FIT_STEP_TOL;
  }
  __device__ inline void keep() { scale = scale_t; }
  // A refused pose has scale 1.
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    int status = st.status;
    float scale_info = 0.f;
    if (!st.refused && !fixed) {
      // ---- the scale information at the accepted state.  After an accepted last trial LDS holds that state (model at its
      // scale, frames, landmarks) and the normal matrix is the one before it: linearise once more.  After a rejected one the
      // normal matrix is the accepted state's already, and nothing else is needed.
      if (st.fresh) fit_linearise(*this, S, lane, st);
      float pivot = 0.f;                              // stays 0 when a pivot is not positive and finite
      fit_solve<NP, LD, false>(S, lane, FITS_SCALE_INFO_LAMBDA, fit_diag<NP>(S, lane), pivot);
      scale_info = uniform(pivot);
      if (scale <= FITS_SCALE_MIN || scale >= FITS_SCALE_MAX) status |= FITS_AT_BOUND;
    }
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
