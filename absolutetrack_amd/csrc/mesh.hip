// Batched linear blend skinning of a hand mesh, with optional per-vertex normals, fp32.
// Replaces lib/common/hand_skinning.py:56-67,130-186 (_lbs, _get_skinned_vertices, _skin_points) for points = the model's
// mesh_vertices [V,3] and skin_mat = its dense_bone_weights [V,17]: skin_landmarks (fk.hip) is the 21-point instance of the
// same function.  The 17 skinning frames are those of fk.hip - the same code (skinning_frames_lds, ut_fk.h).
// Per pose: ~0.9 KB in, 12 V bytes out (24 V with normals; 9.5 / 19 KB for the 788-vertex hand): bound by the output
// stream, so the posed vertices go out as whole 16-byte lanes from LDS.
#include "ut_fk.h"
#include "ut_kernels.h"

namespace ut {

// One workgroup of 256 threads per pose.
//  (1, 2) skinning frames in LDS (ut_fk.h).
//  (3) vertices strided over the workgroup.  A vertex is two float4: (x, y, z, four bone indices as bytes) and four
//      weights; the slots are sorted by ascending bone, so the sum runs in the order of the reference's dense sum over
//      frames (_lbs: matmul(...).sum(dim=2)) with its zero terms left out, and (p, 1) is scaled by the weight first
//      (_get_skinned_vertices).  The posed vertex stays in LDS (s_pos) and the whole pose is stored afterwards, coalesced.
//  (4) normals, when asked for: a gather over the vertex -> incident-triangle CSR built at pack time, each entry the
//      triangle's other two vertices in winding order (v, a, b): n(v) = normalise(sum cross(p[a] - p[v], p[b] - p[v])),
//      i.e. area-weighted, summed in CSR order, negated where the pose is mirrored (the reflection flips the winding).
//      No atomics: a vertex's normal is one thread's sum in a fixed order.  256 normals at a time go through an LDS
//      stage so that they leave coalesced as well.
// No private array is indexed dynamically: frames and positions are read from LDS.
__global__ __launch_bounds__(256) void skin_mesh_kernel(const float* __restrict__ hand_model, int n_models,
                                                        const float* __restrict__ ja, int ja_stride,
                                                        const float* __restrict__ xf, int xf_stride,
                                                        const int64_t* __restrict__ mirror, float t_scale, int n,
                                                        const float4* __restrict__ verts, const uint32_t* __restrict__ csr_off,
                                                        const uint32_t* __restrict__ csr_ent, int nv,
                                                        float* __restrict__ out_v, float* __restrict__ out_n) {
  __shared__ float s_local[1][20][12];
  __shared__ float s_frame[1][17][12];
  __shared__ float s_stage[256 * 3];
  extern __shared__ float4 s_dyn[];              // posed vertices, [nv][3] floats
  float* s_pos = reinterpret_cast<float*>(s_dyn);
  const int tid = threadIdx.x;
  const int i = blockIdx.x;                      // grid = n poses
  skinning_frames_lds<1>(s_local, s_frame, BatchPoses{hand_model, n_models, ja, ja_stride, xf, xf_stride, mirror, t_scale}, n, i);
  // ---- phase 3: linear blend skinning of the vertices
  for (int v = tid; v < nv; v += 256) {
    const float4 pb = verts[2 * v];
    const float4 w4 = verts[2 * v + 1];
    const uint32_t bones = __float_as_uint(pb.w);
    float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float w = k == 0 ? w4.x : k == 1 ? w4.y : k == 2 ? w4.z : w4.w;
      if (w != 0.f) {
        const float* t = s_frame[0][(bones >> (8 * k)) & 0xFFu];
        const float qx = pb.x * w, qy = pb.y * w, qz = pb.z * w;   // (p,1) * w, as the reference scales first
        ax += t[0] * qx + t[1] * qy + t[2] * qz + t[3] * w;
        ay += t[4] * qx + t[5] * qy + t[6] * qz + t[7] * w;
        az += t[8] * qx + t[9] * qy + t[10] * qz + t[11] * w;
      }
    }
    s_pos[3 * v] = ax; s_pos[3 * v + 1] = ay; s_pos[3 * v + 2] = az;
  }
  __syncthreads();
  const int nf = 3 * nv;
  {
    float* o = out_v + (size_t)i * nf;
    if ((nf & 3) == 0 && (reinterpret_cast<uintptr_t>(out_v) & 15) == 0) {   // every pose starts on a 16-byte boundary
      float4* o4 = reinterpret_cast<float4*>(o);
      for (int j = tid; j < (nf >> 2); j += 256) o4[j] = s_dyn[j];
    } else {
      for (int j = tid; j < nf; j += 256) o[j] = s_pos[j];
    }
  }
  if (!out_n) return;
  // ---- phase 4: area-weighted vertex normals
  const bool flip = mirror && mirror[i] == 1;
  float* on = out_n + (size_t)i * nf;
  for (int v0 = 0; v0 < nv; v0 += 256) {
    const int v = v0 + tid;
    if (v < nv) {
      const float px = s_pos[3 * v], py = s_pos[3 * v + 1], pz = s_pos[3 * v + 2];
      float nx = 0.f, ny = 0.f, nz = 0.f;
      const uint32_t e1 = csr_off[v + 1];
      for (uint32_t e = csr_off[v]; e < e1; ++e) {
        const uint32_t ab = csr_ent[e];
        const float* pa = s_pos + 3 * (ab & 0xFFFFu);
        const float* pc = s_pos + 3 * (ab >> 16);
        const float ux = pa[0] - px, uy = pa[1] - py, uz = pa[2] - pz;
        const float wx = pc[0] - px, wy = pc[1] - py, wz = pc[2] - pz;
        nx += uy * wz - uz * wy;
        ny += uz * wx - ux * wz;
        nz += ux * wy - uy * wx;
      }
      if (flip) { nx = -nx; ny = -ny; nz = -nz; }
      const float l2 = nx * nx + ny * ny + nz * nz;
      const float inv = l2 > 0.f ? 1.0f / sqrtf(l2) : 0.f;
      s_stage[3 * tid] = nx * inv; s_stage[3 * tid + 1] = ny * inv; s_stage[3 * tid + 2] = nz * inv;
    }
    __syncthreads();
    const int cnt = 3 * min(256, nv - v0);
    for (int j = tid; j < cnt; j += 256) on[3 * v0 + j] = s_stage[j];
    __syncthreads();
  }
}

hipError_t launch_skin_mesh(const float* hand_model, int n_models, const float* ja, int ja_stride, const float* xf,
                            int xf_stride, const int64_t* mirror, float t_scale, int n, const void* verts,
                            const uint32_t* csr_off, const uint32_t* csr_ent, int nv, float* out_v, float* out_n,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (nv <= 0 || nv > MESH_MAX_VERTICES) return hipErrorInvalidValue;
  const size_t lds = ((size_t)nv * 12 + 15) / 16 * 16;
  hipLaunchKernelGGL(skin_mesh_kernel, dim3(n), dim3(256), lds, s, hand_model, n_models, ja, ja_stride, xf, xf_stride,
                     mirror, t_scale, n, (const float4*)verts, csr_off, csr_ent, nv, out_v, out_n);
  return hipGetLastError();
}

}  // namespace ut
