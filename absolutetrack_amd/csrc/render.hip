// The tracked hand back in the images: world points into camera windows (ut_project_points) and the posed mesh rasterised
// into the 96x96 crop cameras the network reads (ut_render_mesh): depth, winning triangle, flat headlight shading.
// Replaces the host loops of the reference's scripts: camera.eye_to_window(camera.world_to_eye(...)) per camera
// (run_eval_known_skeleton_analysis.py:296-358, lib/common/camera.py:76-94,296-312); the rasteriser has no counterpart.
// Every multiply and add of this file rounds on its own (no contraction), like the numpy statements it is tested against.
#pragma clang fp contract(off)
#include "ut_camera.h"
#include "ut_kernels.h"

namespace ut {

// ---------------------------------------------------------------- points -> windows
// One thread per (pose, view, point).  fp64 throughout, the reference's order: world_to_eye (R^T (p - t)), project,
// distort.evaluate, * f + c.  A view whose cam_rows entry is -1 is unused: zeros.  An entry outside [-1, n_rows) sets
// UT_BAD_SRC_INDEX and writes nothing.
__global__ __launch_bounds__(256) void project_points_kernel(ProjectArgs g) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)g.n * g.max_views * g.n_points;
  if (idx >= total) return;
  const int p = (int)(idx % g.n_points);
  const long long iv = idx / g.n_points;
  const int i = (int)(iv / g.max_views);
  const int row = g.cam_rows[iv];
  if (row < -1 || row >= g.n_rows) {
    if (p == 0) atomicOr(g.status, UT_BAD_SRC_INDEX);
    return;
  }
  double win[2] = {0.0, 0.0}, ez = 0.0;
  unsigned flags = 0;
  if (row >= 0) {
    const float* pt = g.points + (size_t)i * g.point_stride + 3 * p;
    const double w[3] = {(double)pt[0], (double)pt[1], (double)pt[2]};
    double e[3];
    if (g.kind == PROJECT_FISHEYE62) {
      const double* cam = g.table + (size_t)row * 32;
      world_to_eye_d(cam, w, e);
      fisheye_project_d(cam, e, win);
    } else {                       // pinhole crop camera: fx fy cx cy | R(9) t(3) of camera_to_world
      const double* cp = g.table + (size_t)row * 24;
      const double* r = cp + 4;
      const double dx = w[0] - cp[13], dy = w[1] - cp[14], dz = w[2] - cp[15];
      e[0] = r[0] * dx + r[3] * dy + r[6] * dz;
      e[1] = r[1] * dx + r[4] * dy + r[7] * dz;
      e[2] = r[2] * dx + r[5] * dy + r[8] * dz;
      win[0] = e[0] / e[2] * cp[0] + cp[2];
      win[1] = e[1] / e[2] * cp[1] + cp[3];
    }
    ez = e[2];
    if (ez > 0) flags |= 1u;
    if (win[0] >= 0 && win[0] < (double)g.width && win[1] >= 0 && win[1] < (double)g.height) flags |= 2u;
  }
  g.window[2 * idx] = win[0];
  g.window[2 * idx + 1] = win[1];
  g.eye_z[idx] = ez;
  g.flags[idx] = (uint8_t)flags;
}

hipError_t launch_project_points(const ProjectArgs& g, hipStream_t s) {
  const long long total = (long long)g.n * g.max_views * g.n_points;
  if (total <= 0) return hipSuccess;
  if (total > (1ll << 38)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(project_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g);
  return hipGetLastError();
}

// ---------------------------------------------------------------- mesh -> crop images
constexpr int RN = RENDER_CROP;                 // 96
constexpr int RN_BAND = RN / 2;                 // rows per pass
constexpr int RN_PLANE = RN_BAND * RN;          // 4608 pixels per pass
constexpr unsigned long long RN_EMPTY = ~0ull;
constexpr double RN_NEAR = 1e-4;                // lib/common/crop.py:25

__global__ __launch_bounds__(256) void render_check_kernel(const int64_t* __restrict__ sample_range, int n, int n_crops,
                                                           int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long r0 = sample_range[2 * i], r1 = sample_range[2 * i + 1];
  if (r0 < 0 || r1 > n_crops || r1 < r0 || r1 - r0 > 2) atomicOr(status, UT_BAD_SAMPLE_RANGE);
}

// One workgroup of 256 threads per (pose, view slot): blockIdx.x = 2 * pose + slot; the crop is sample_range[pose][0] + slot.
//  (1) the pose's V vertices through the crop camera in fp64 (the fp32 vertex widened exactly; R^T (p - t), / z, * f + c),
//      kept in LDS as fp32 (x, y, 1 / z); a vertex with z < 1e-4 (or not a number) is marked with 1 / z = -1.
//  (2) the image in two passes of 48 rows.  A pass owns a plane of 48 x 96 64-bit words in LDS, depth bits << 32 | triangle.
//      Triangles are strided over the threads; each walks the pixels of its bounding box inside the pass and offers its word
//      with one LDS atomicMin per covered pixel.  Depths are positive, so their bit patterns order like the numbers, and the
//      smaller triangle index wins on equal depth: the minimum does not depend on the order of arrival.
//      A triangle with a marked vertex is skipped whole; one whose fp32 area is zero, infinite or not a number (a vertex that
//      projects to a NaN or an infinity, or an overflowing product) covers nothing.  No culling: a triangle is brought to
//      positive area by exchanging two vertices first (crop cameras of right hands are mirrored).  With
//         E_ab(p) = (xb - xa) (py - ya) - (yb - ya) (px - xa)
//      evaluated from the edge's own start vertex, a pixel centre is covered when E_01, E_12, E_20 >= 0, and a zero counts only
//      on a top or left edge: yb - ya < 0, or yb == ya and xb - xa > 0 (y grows downwards).  1 / z is linear on the screen:
//         1 / z(p) = w0 + (E_20 (w1 - w0) + E_01 (w2 - w0)) / area.
//  (3) the plane leaves as 16-byte stores of row pieces: depth (+inf on background), triangle (-1), shade (0), where shade is
//      round(255 |n . c| / (|n| |c|)) of the winning triangle: n its face normal, c its centroid, both in eye space rebuilt
//      from (x, y, 1 / z).  |n . c| is the same in a mirrored camera.
__global__ __launch_bounds__(256) void render_mesh_kernel(RenderArgs g) {
  if (((volatile const int*)g.status)[0] & UT_STATUS_ERRORS) return;
  const int i = blockIdx.x >> 1, slot = blockIdx.x & 1;
  const long long r0 = g.sample_range[2 * i], r1 = g.sample_range[2 * i + 1];
  if (r0 < 0 || r1 > g.n_crops || r1 < r0 || r1 - r0 > 2) return;      // render_check_kernel has reported it
  if (slot >= r1 - r0) return;
  const int crop = (int)r0 + slot;
  __shared__ unsigned long long s_plane[RN_PLANE];
  extern __shared__ float s_vert[];                                     // [nv][3]: x, y, 1 / z
  const int tid = threadIdx.x;
  const double* cp = g.crop_params + (size_t)crop * 24;
  const float fx = (float)cp[0], fy = (float)cp[1], cx = (float)cp[2], cy = (float)cp[3];
  // ---- (1)
  {
    const double f0 = cp[0], f1 = cp[1], c0 = cp[2], c1 = cp[3];
    const double* r = cp + 4;
    const double t0 = cp[13], t1 = cp[14], t2 = cp[15];
    const float* vin = g.vertices + (size_t)i * g.nv * 3;
    for (int v = tid; v < g.nv; v += 256) {
      const double dx = (double)vin[3 * v] - t0, dy = (double)vin[3 * v + 1] - t1, dz = (double)vin[3 * v + 2] - t2;
      const double ex = r[0] * dx + r[3] * dy + r[6] * dz;
      const double ey = r[1] * dx + r[4] * dy + r[7] * dz;
      const double ez = r[2] * dx + r[5] * dy + r[8] * dz;
      float x = 0.f, y = 0.f, w = -1.f;
      if (ez >= RN_NEAR) {
        x = (float)(ex / ez * f0 + c0);
        y = (float)(ey / ez * f1 + c1);
        w = (float)(1.0 / ez);
      }
      s_vert[3 * v] = x; s_vert[3 * v + 1] = y; s_vert[3 * v + 2] = w;
    }
  }
  for (int band = 0; band < 2; ++band) {
    const int row_lo = band * RN_BAND, row_hi = row_lo + RN_BAND - 1;
    __syncthreads();                                                     // vertices written / previous plane stored
    for (int k = tid; k < RN_PLANE; k += 256) s_plane[k] = RN_EMPTY;
    __syncthreads();
    // ---- (2)
    for (int t = tid; t < g.nt; t += 256) {
      const int4 tv = g.tris[t];
      const float* a = s_vert + 3 * tv.x;
      const float* b = s_vert + 3 * tv.y;
      const float* c = s_vert + 3 * tv.z;
      const float x0 = a[0], y0 = a[1], w0 = a[2];
      float x1 = b[0], y1 = b[1], w1 = b[2];
      float x2 = c[0], y2 = c[1], w2 = c[2];
      if (w0 < 0.f || w1 < 0.f || w2 < 0.f) continue;
      float area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
      if (!(fabsf(area) > 0.f && fabsf(area) < INFINITY)) continue;     // zero area, infinite (fp32 overflow), or not a number
      if (area < 0.f) {
        float s;
        s = x1; x1 = x2; x2 = s;
        s = y1; y1 = y2; y2 = s;
        s = w1; w1 = w2; w2 = s;
        area = -area;
      }
      const int px_lo = (int)ceilf(fmaxf(fminf(fminf(x0, x1), x2), 0.f));
      const int px_hi = (int)floorf(fminf(fmaxf(fmaxf(x0, x1), x2), (float)(RN - 1)));
      const int py_lo = (int)ceilf(fmaxf(fminf(fminf(y0, y1), y2), (float)row_lo));
      const int py_hi = (int)floorf(fminf(fmaxf(fmaxf(y0, y1), y2), (float)row_hi));
      if (px_lo > px_hi || py_lo > py_hi || px_lo < 0 || px_hi > RN - 1 || py_lo < row_lo || py_hi > row_hi) continue;
      const float d01x = x1 - x0, d01y = y1 - y0, d12x = x2 - x1, d12y = y2 - y1, d20x = x0 - x2, d20y = y0 - y2;
      const bool tl01 = d01y < 0.f || (d01y == 0.f && d01x > 0.f);
      const bool tl12 = d12y < 0.f || (d12y == 0.f && d12x > 0.f);
      const bool tl20 = d20y < 0.f || (d20y == 0.f && d20x > 0.f);
      const float dw1 = w1 - w0, dw2 = w2 - w0;
      for (int py = py_lo; py <= py_hi; ++py) {
        const float fy_ = (float)py;
        for (int px = px_lo; px <= px_hi; ++px) {
          const float fx_ = (float)px;
          const float e01 = d01x * (fy_ - y0) - d01y * (fx_ - x0);
          const float e12 = d12x * (fy_ - y1) - d12y * (fx_ - x1);
          const float e20 = d20x * (fy_ - y2) - d20y * (fx_ - x2);
          const bool in = (e01 > 0.f || (e01 == 0.f && tl01)) && (e12 > 0.f || (e12 == 0.f && tl12)) &&
                          (e20 > 0.f || (e20 == 0.f && tl20));
          if (!in) continue;
          const float iz = w0 + (e20 * dw1 + e01 * dw2) / area;
          const float z = 1.0f / iz;
          if (!(z > 0.f && z < INFINITY)) continue;
          const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)t;
          atomicMin(&s_plane[(py - row_lo) * RN + px], key);
        }
      }
    }
    __syncthreads();
    // ---- (3) four pixels per thread; the shades of four neighbouring threads leave as one 16-byte store
    for (int base = 0; base < RN_PLANE / 4; base += 256) {
      const int q = base + tid;
      const bool active = q < RN_PLANE / 4;
      float dep[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
      int win[4] = {-1, -1, -1, -1};
      unsigned sh = 0;
      if (active) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned long long word = s_plane[4 * q + k];
          if (word == RN_EMPTY) continue;
          const int t = (int)(unsigned)(word & 0xFFFFFFFFull);
          dep[k] = __uint_as_float((unsigned)(word >> 32));
          win[k] = t;
          const int4 tv = g.tris[t];
          float p[3][3];
          const int vi[3] = {tv.x, tv.y, tv.z};
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const float* sv = s_vert + 3 * vi[m];
            const float z = 1.0f / sv[2];
            p[m][0] = (sv[0] - cx) / fx * z;
            p[m][1] = (sv[1] - cy) / fy * z;
            p[m][2] = z;
          }
          const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
          const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
          const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
          const float gx = (p[0][0] + p[1][0] + p[2][0]) / 3.0f, gy = (p[0][1] + p[1][1] + p[2][1]) / 3.0f,
                      gz = (p[0][2] + p[1][2] + p[2][2]) / 3.0f;
          const float nn = nx * nx + ny * ny + nz * nz, gg = gx * gx + gy * gy + gz * gz;
          float s = 0.f;
          if (nn > 0.f && gg > 0.f) s = fabsf(nx * gx + ny * gy + nz * gz) / sqrtf(nn * gg);
          const unsigned level = (unsigned)rintf(255.0f * fminf(s, 1.0f));
          sh |= level << (8 * k);
        }
      }
      const int lane = tid & 63, lead = lane & ~3;
      uint4 sh4;
      sh4.x = __shfl(sh, lead);
      sh4.y = __shfl(sh, lead + 1);
      sh4.z = __shfl(sh, lead + 2);
      sh4.w = __shfl(sh, lead + 3);
      if (active) {
        const size_t o = (size_t)crop * (RN * RN) + (size_t)row_lo * RN + 4 * (size_t)q;
        if (g.depth) *reinterpret_cast<float4*>(g.depth + o) = make_float4(dep[0], dep[1], dep[2], dep[3]);
        if (g.tri) *reinterpret_cast<int4*>(g.tri + o) = make_int4(win[0], win[1], win[2], win[3]);
        if (g.shade && lane == lead) *reinterpret_cast<uint4*>(g.shade + o) = sh4;
      }
    }
  }
}

// the sample_range check, stream ordered in front of the drawing launch (which returns at once when the sticky word holds an error)
hipError_t launch_render_check(const RenderArgs& g, hipStream_t s) {
  if (g.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(render_check_kernel, dim3((g.n + 255) / 256), dim3(256), 0, s, g.sample_range, g.n, g.n_crops, g.status);
  return hipGetLastError();
}

hipError_t launch_render_mesh(const RenderArgs& g, hipStream_t s) {
  if (g.n <= 0) return hipSuccess;
  if (g.nv <= 0 || g.nv > RENDER_MAX_VERTICES || g.nt <= 0 || g.n > (1 << 30)) return hipErrorInvalidValue;
  const size_t lds = ((size_t)g.nv * 12 + 15) / 16 * 16;
  hipLaunchKernelGGL(render_mesh_kernel, dim3(2 * (unsigned)g.n), dim3(256), lds, s, g);
  return hipGetLastError();
}

}  // namespace ut
