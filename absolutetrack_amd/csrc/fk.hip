// Batched forward kinematics + linear blend skinning of the 21 hand landmarks, fp32.
// Replaces lib/common/hand_skinning.py:17-209 (skin_landmarks) and the rotation exponential it
// takes from pytorch3d (so3_exp_map, eps = 1e-4: theta = sqrt(max(|v|^2, eps)),
// R = I + sin(theta)/theta K + (1-cos(theta))/theta^2 K^2).
// ~4 kFLOP and 0.9 KB per pose - latency bound, not a matrix-core shape.
// 17 skinning frames = [wrist, wrist, then per finger W*L0*L1, W*L0*L1*L2, W*L0*L1*L2*L3]
// (the one-joint product is dropped, hand_skinning.py:32).
#include "ut_fk.h"
#include "ut_kernels.h"

namespace ut {

// Three phases per block of FK_P poses, all operands through LDS so that no thread indexes a private array
// dynamically: (1) one thread per (pose, joint) builds the joint's local transform (sin/cos), (2) one thread per
// (pose, finger) multiplies the chain wrist*L0*L1*L2*L3 and keeps the frames after 2, 3, 4 joints, (3) one thread
// per (pose, landmark) blends.  Phases 1, 2 are skinning_frames_lds and phase 3 is blend_landmark of ut_fk.h, which
// mesh.hip (frames) and cropgen.hip (frames and blend, three crop poses per candidate) call as well.
constexpr int FK_P = 12;

__global__ __launch_bounds__(256) void fk_kernel(const float* __restrict__ hand_model, int n_models,
                                                 const float* __restrict__ ja, int ja_stride,
                                                 const float* __restrict__ xf, int xf_stride,
                                                 const int64_t* __restrict__ mirror, float t_scale, int n,
                                                 float* __restrict__ out) {
  __shared__ float s_local[FK_P][20][12];
  __shared__ float s_frame[FK_P][17][12];
  const int tid = threadIdx.x;
  const int base = blockIdx.x * FK_P;
  const BatchPoses poses{hand_model, n_models, ja, ja_stride, xf, xf_stride, mirror, t_scale};
  // ---- phases 1, 2: the skinning frames (ut_fk.h; mesh.hip and cropgen.hip build their frames with the same code)
  skinning_frames_lds<FK_P>(s_local, s_frame, poses, n, base);
  // ---- phase 3: linear blend skinning (ut_fk.h; cropgen.hip blends its crop points with the same code)
  if (tid < FK_P * 21) {
    const int pl = tid / 21, l = tid - pl * 21;
    const int i = base + pl;
    if (i < n) blend_landmark(poses.model(i), l, s_frame[pl], out + (size_t)i * 63 + 3 * l);
  }
}

hipError_t launch_fk(const float* hand_model, int n_models, const float* ja, int ja_stride, const float* xf,
                     int xf_stride, const int64_t* mirror, float t_scale, int n, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fk_kernel, dim3((n + FK_P - 1) / FK_P), dim3(256), 0, s, hand_model, n_models, ja, ja_stride, xf,
                     xf_stride, mirror, t_scale, n, out);
  return hipGetLastError();
}

}  // namespace ut
