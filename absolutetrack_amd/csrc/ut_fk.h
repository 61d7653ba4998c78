// Device-side forward kinematics + linear blend skinning shared by fk.hip, mesh.hip and cropgen.hip.
// See fk.hip for the reference citations (lib/common/hand_skinning.py:17-209, pytorch3d so3_exp_map).
#pragma once
#include <hip/hip_runtime.h>

namespace ut {

struct M34 { float m[12]; };   // rows 0..2 of a 4x4 rigid/affine transform, row major

__device__ inline M34 mul34(const M34& a, const M34& b) {
  M34 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = a.m[4 * i] * b.m[j];
      s = fmaf(a.m[4 * i + 1], b.m[4 + j], s);
      s = fmaf(a.m[4 * i + 2], b.m[8 + j], s);
      if (j == 3) s += a.m[4 * i + 3];
      c.m[4 * i + j] = s;
    }
  }
  return c;
}

__device__ inline M34 joint_local(const float* axis, const float* rest, float angle) {
  const float vx = axis[0] * angle, vy = axis[1] * angle, vz = axis[2] * angle;
  const float n2 = vx * vx + vy * vy + vz * vz;
  const float th = sqrtf(fmaxf(n2, 1e-4f));
  const float inv = 1.0f / th;
  const float f1 = inv * sinf(th);
  const float f2 = inv * inv * (1.0f - cosf(th));
  // K = hat(v); K^2 has -(vy^2+vz^2) etc. on the diagonal and vi*vj off it
  float r[9];
  r[0] = 1.0f - f2 * (vy * vy + vz * vz);
  r[1] = -f1 * vz + f2 * (vx * vy);
  r[2] = f1 * vy + f2 * (vx * vz);
  r[3] = f1 * vz + f2 * (vx * vy);
  r[4] = 1.0f - f2 * (vx * vx + vz * vz);
  r[5] = -f1 * vx + f2 * (vy * vz);
  r[6] = -f1 * vy + f2 * (vx * vz);
  r[7] = f1 * vx + f2 * (vy * vz);
  r[8] = 1.0f - f2 * (vx * vx + vy * vy);
  M34 l;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    l.m[4 * i] = r[3 * i]; l.m[4 * i + 1] = r[3 * i + 1]; l.m[4 * i + 2] = r[3 * i + 2];
    l.m[4 * i + 3] = rest[i] - (r[3 * i] * rest[0] + r[3 * i + 1] * rest[1] + r[3 * i + 2] * rest[2]);
  }
  return l;
}


// The poses of a batch as skinning_frames_lds reads them (fk.hip, mesh.hip): pose i takes its 20 joint angles from
// ja[i * ja_stride], its wrist transform (rows 0..2, row major) from xf[i * xf_stride] and row i of the packed models
// (row 0 when there is one model); its translation is multiplied by t_scale and the hand is mirrored where mirror[i] == 1.
struct BatchPoses {
  const float* hand_model; int n_models;
  const float* ja; int ja_stride;
  const float* xf; int xf_stride;
  const int64_t* mirror;
  float t_scale;
  __device__ const float* model(int i) const { return hand_model + (size_t)(n_models == 1 ? 0 : i) * 321; }
  __device__ float angle(int i, int q) const { return ja[(size_t)i * ja_stride + q]; }
  __device__ const float* wrist(int i) const { return xf + (size_t)i * xf_stride; }
  __device__ bool mirrored(int i) const { return mirror && mirror[i] == 1; }
};

// The 17 skinning frames of P poses (base .. base + P - 1, those below n) into s_frame, by a workgroup of at least 21 * P
// threads, operands through LDS so that no thread indexes a private array dynamically: (1) one thread per (pose, joint)
// builds the joint's local transform (sin/cos) while one per pose writes the wrist frames (slots 0, 1: translation times
// t_scale, column 0 negated where the pose is mirrored), (2) one thread per (pose, finger) multiplies the chain
// wrist*L0*L1*L2*L3 and keeps the frames after 2, 3, 4 joints.  Ends on a barrier: every thread of the workgroup must call
// it, and may read s_frame when it returns.  `poses` says where pose i's model row, angles, wrist, mirror flag and t_scale
// come from (BatchPoses above; cropgen.hip has its own for the three crop poses of a candidate).  Shared by fk.hip
// (landmarks), mesh.hip (mesh vertices) and cropgen.hip (crop points): one arithmetic, one order.
template <int P, class Poses>
__device__ inline void skinning_frames_lds(float (&s_local)[P][20][12], float (&s_frame)[P][17][12], const Poses& poses,
                                           int n, int base) {
  const int tid = threadIdx.x;
  // ---- phase 1: joint local transforms (20 per pose) and the wrist frames (slots 0, 1)
  if (tid < P * 20) {
    const int pl = tid / 20, q = tid - pl * 20;
    const int i = base + pl;
    if (i < n) {
      const float* hm = poses.model(i);
      const M34 l = joint_local(hm + 3 * q, hm + 66 + 3 * q, poses.angle(i, q));
#pragma unroll
      for (int k = 0; k < 12; ++k) s_local[pl][q][k] = l.m[k];
    }
  } else if (tid < P * 20 + P) {
    const int pl = tid - P * 20;
    const int i = base + pl;
    if (i < n) {
      const float* x = poses.wrist(i);
      M34 w;
#pragma unroll
      for (int k = 0; k < 12; ++k) w.m[k] = x[k];
      w.m[3] *= poses.t_scale; w.m[7] *= poses.t_scale; w.m[11] *= poses.t_scale;
      if (poses.mirrored(i)) { w.m[0] = -w.m[0]; w.m[4] = -w.m[4]; w.m[8] = -w.m[8]; }
#pragma unroll
      for (int k = 0; k < 12; ++k) { s_frame[pl][0][k] = w.m[k]; s_frame[pl][1][k] = w.m[k]; }
    }
  }
  __syncthreads();
  // ---- phase 2: finger chains
  if (tid < P * 5) {
    const int pl = tid / 5, f = tid - pl * 5;
    if (base + pl < n) {
      M34 t;
#pragma unroll
      for (int k = 0; k < 12; ++k) t.m[k] = s_frame[pl][0][k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        M34 l;
#pragma unroll
        for (int k = 0; k < 12; ++k) l.m[k] = s_local[pl][4 * f + j][k];
        t = mul34(t, l);
        if (j >= 1) {
#pragma unroll
          for (int k = 0; k < 12; ++k) s_frame[pl][2 + 3 * f + (j - 1)][k] = t.m[k];
        }
      }
    }
  }
  __syncthreads();
}

// What the pose fit (fit.hip) needs beyond the 17 frames: the chain of finger f as skinning_frames_lds multiplies it (same
// products, same order, so the frames are the same bits), keeping the prefix frame in front of every joint as well -
// prefix[4 f + j] = W L0 .. L(j-1), the frame joint j of the finger turns in - next to frame[2 + 3 f + (j - 1)] = W L0 .. Lj
// for j >= 1.  local: the 20 joint transforms of the pose (joint_local), wrist: its wrist frame (slot 0).  One thread per
// finger; the caller orders the LDS accesses around it.
__device__ inline void finger_chain_with_prefixes(const M34& wrist, const float (&local)[20][12], int f,
                                                  float (&prefix)[20][12], float (&frame)[17][12]) {
  M34 t = wrist;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < 12; ++k) prefix[4 * f + j][k] = t.m[k];
    M34 l;
#pragma unroll
    for (int k = 0; k < 12; ++k) l.m[k] = local[4 * f + j][k];
    t = mul34(t, l);
    if (j >= 1) {
#pragma unroll
      for (int k = 0; k < 12; ++k) frame[2 + 3 * f + (j - 1)][k] = t.m[k];
    }
  }
}

// Joint q in the world, from its prefix frame p (finger_chain_with_prefixes): omega = the frame's linear part times the
// rotation axis, c_w = the frame applied to the joint's rest position.  d(T x)/d(angle q) = s * omega x (T x - c_w) for
// every frame T whose product contains the joint, s = the determinant of the wrist's linear part.
__device__ inline void joint_axis_in_world(const float* p, const float* axis, const float* rest, float* omega, float* c_w) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    omega[i] = p[4 * i] * axis[0] + p[4 * i + 1] * axis[1] + p[4 * i + 2] * axis[2];
    c_w[i] = p[4 * i] * rest[0] + p[4 * i + 1] * rest[1] + p[4 * i + 2] * rest[2] + p[4 * i + 3];
  }
}

// Landmark l of one pose into o[0..2]: linear blend skinning over the pose's 17 frames (in LDS, from skinning_frames_lds),
// frames visited in ascending order like the dense reference sum.  hm: packed hand model (321 floats, see
// include/umetrack_hip.h).
__device__ inline void blend_landmark(const float* __restrict__ hm, int l, const float (&frames)[17][12],
                                      float* __restrict__ o) {
  const float* lm = hm + 132;
  const float* wts = hm + 195;
  const float* idx = hm + 258;
  const float px = lm[3 * l], py = lm[3 * l + 1], pz = lm[3 * l + 2];
  const float w0 = wts[3 * l], w1 = wts[3 * l + 1], w2 = wts[3 * l + 2];
  const int i0 = (int)idx[3 * l], i1 = (int)idx[3 * l + 1], i2 = (int)idx[3 * l + 2];
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int f = 0; f < 17; ++f) {
    // dense skinning weight of frame f: the last non-zero entry naming it wins
    float w = 0.f;
    if (w0 != 0.f && i0 == f) w = w0;
    if (w1 != 0.f && i1 == f) w = w1;
    if (w2 != 0.f && i2 == f) w = w2;
    if (w != 0.f) {
      const float* t = frames[f];
      const float qx = px * w, qy = py * w, qz = pz * w;   // (p,1) * w, as the reference scales first
      ax += t[0] * qx + t[1] * qy + t[2] * qz + t[3] * w;
      ay += t[4] * qx + t[5] * qy + t[6] * qz + t[7] * w;
      az += t[8] * qx + t[9] * qy + t[10] * qz + t[11] * w;
    }
  }
  o[0] = ax; o[1] = ay; o[2] = az;
}

}  // namespace ut
