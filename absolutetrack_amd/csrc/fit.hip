// Batched inverse kinematics, fp32: the pose (20 joint angles + a rigid wrist) whose 21 landmarks - fk.hip's function,
// lib/common/hand_skinning.py:189-209 - meet given targets.  The reference has no counterpart; the yardstick is the float64
// restatement in tests/fit_cases.py.
//
// The solver is ut_fit_dev.h's fit_pose(), on 26 parameters; this file is its plainest cost, sum_l w_l |landmark_l -
// target_l|^2 with a scalar weight per landmark: Jacobian rows scaled by sqrt(weight), the isotropic cost fit_eval sums, the
// info row (rms over the weights' sum).  ~60 kFLOP per iteration and pose: latency bound like fk.hip, not a matrix-core
// shape.  One wave per pose, FIT_P poses per workgroup.
#include "ut_fit_dev.h"

namespace ut {

constexpr int FIT_P = 4;         // poses (waves) per workgroup

struct FitLds {                  // one wave's region, 15064 bytes: FIT_P of them stay inside the 64 KB a workgroup gets
  float hm[321];                 // the pose's packed model
  float local[20][12];           // joint transforms of the last evaluated state
  float prefix[20][12];          // W L0 .. L(j-1) in front of joint 4 f + j
  float frame[17][12];           // skinning frames
  float omega[20][3], cw[20][3]; // joint axes and centres in the world (linearisation)
  float jl[63 * 27];             // J while the normal matrix is formed, then the Cholesky factor L [26][27]
  float a[27][27];               // lower triangle of [J r]^T [J r]: A = J^T J, row 26 = g = J^T r
  float ang[20], ang_t[20];      // accepted and trial angles
  float wrist[12], wrist_t[12];  // accepted and trial wrist frame (translation in target units, column 0 negated if mirrored)
  float p[21][3];                // landmarks of the last evaluated state
  float target[21][3], w[21];    // targets (0 where the weight is 0) and weights
};
static_assert(sizeof(FitLds) == 15064 && sizeof(FitLds) * FIT_P <= 65536, "a workgroup's static LDS");

struct FitCost {
  using Lds = FitLds;
  static constexpr int NP = 26, LD = 27;
  const FitArgs& a;

  __device__ inline bool load(Lds&, int i, int, int lane, float& wl, bool& used) {
    return fit_scalar_weight(a.weights, i, lane, wl, used);
  }
  __device__ inline float row_scale(const Lds& S, int lane) { return sqrtf(S.w[lane]); }
  __device__ inline void finish_rows(Lds&, int, float*, float, float, float, float) {}
  __device__ inline float cost(const Lds&, int, bool, float isotropic) { return isotropic; }
  __device__ inline bool trial(Lds&, int, float) { return true; }
  __device__ inline void keep() {}
  // rms over the weights' sum
  __device__ inline void report(Lds&, int i, int lane, const FitState& st) {
    if (a.info && lane == 0) fit_store_info(a.info + (size_t)i * 4, st, st.wsum, st.status);
  }
};

__global__ __launch_bounds__(64 * FIT_P) void fit_pose_kernel(const FitArgs a) {
  __shared__ FitLds s_all[FIT_P];
  const int i = blockIdx.x * FIT_P + (threadIdx.x >> 6);
  if (i >= a.pose.n) return;                          // whole waves leave; nobody waits for them
  FitCost cost{a};
  fit_pose(cost, s_all[threadIdx.x >> 6], a.pose, i, threadIdx.x & 63);
}

hipError_t launch_fit_pose(const FitArgs& a, hipStream_t s) {
  if (a.pose.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fit_pose_kernel, dim3((a.pose.n + FIT_P - 1) / FIT_P), dim3(64 * FIT_P), 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
