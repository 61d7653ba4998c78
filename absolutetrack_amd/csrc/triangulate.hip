// Points from views (ut_triangulate_points, include/umetrack_hip_triangulate.h; ut_triangulate_points_info,
// include/umetrack_hip_info.h): the inverse of ut_project_points.  Window coordinates of one point in several cameras -> the
// world point, its reprojection residuals and its uncertainty - as one number, or as the factor of its 3 x 3 information.
// One thread per (pose, point); fp64 throughout.  Per thread: a linear start from the views' rays, then Levenberg-Marquardt on
// the reprojection error through the exact forward model (world_to_eye_d + fisheye_project_d of ut_camera.h, or the pinhole of
// render.hip) with an analytic 2 x 3 Jacobian per view (project_jac and the 3 x 3 Cholesky helpers of ut_camera.h, shared with
// fit_views.hip).  The views are visited in ascending order by a loop bounded by
// max_views (<= TRI_MAX_VIEWS) that reads each view's camera row, window and weight from global memory every time - a pose's
// 21 points share their camera rows, so these loads hit the cache - and keeps only sums in registers: no per-view private
// array, no LDS, no scratch, no atomics but the index check's status bit.  Every multiply and add of this file rounds on
// its own (no contraction), like the numpy restatement it is tested against (tests/triangulate_cases.py).
#pragma clang fp contract(off)
#include "ut_camera.h"
#include "ut_kernels.h"

namespace ut {

namespace {

constexpr double TRI_LAMBDA_START = 1e-6, TRI_LAMBDA_DOWN = 0.1, TRI_LAMBDA_UP = 10.0, TRI_LAMBDA_MIN = 1e-12;
constexpr double TRI_LAMBDA_CONVERGED_MAX = 1.0;   // a small step under heavy damping is a stall, not convergence
constexpr double TRI_STEP_TOL = 1e-12;             // x sqrt(1 + |X|^2)
constexpr double TRI_FLAT_TOL_PX = 1e-11;          // rms residual of a rejected trial this close to the accepted one

// Start ray of a window point: unit direction d in the world; the origin is the camera centre (returned pointer).
template <int KIND>
__device__ inline const double* start_ray(const double* cam, const double* w, double* d) {
  const double* t;
  if (KIND == PROJECT_FISHEYE62) {
    double p[3];
    window_to_world_d(cam, w, p);     // a point at distance 1 from the centre, as the reference unprojects it
    t = cam + 21;
    d[0] = p[0] - t[0]; d[1] = p[1] - t[1]; d[2] = p[2] - t[2];
  } else {
    const double* r = cam + 4;
    t = cam + 13;
    const double qx = (w[0] - cam[2]) / cam[0], qy = (w[1] - cam[3]) / cam[1];
    d[0] = r[0] * qx + r[1] * qy + r[2];
    d[1] = r[3] * qx + r[4] * qy + r[5];
    d[2] = r[6] * qx + r[7] * qy + r[8];
  }
  const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d[0] /= len; d[1] /= len; d[2] /= len;
  return t;
}

struct Normal {         // what one evaluation at a point leaves: cost, H = sum w J^T J, g = sum w J^T r
  double cost;
  Sym3 h;
  double g0, g1, g2;
  bool good;            // finite, and behind no used pinhole view's near plane
};

template <int KIND>
struct View {           // the addresses of one (pose, point)'s per-view inputs
  const TriArgs& a;
  const int32_t* rows;
  const double* win;    // + v * n_points * 2
  const float* wgt;     // + v * n_points, or null
  __device__ const double* cam(int v) const { return a.table + (size_t)rows[v] * (KIND == PROJECT_FISHEYE62 ? 32 : 24); }
  __device__ const double* window(int v) const { return win + (size_t)v * a.n_points * 2; }
  __device__ double weight(int v) const { return wgt ? (double)wgt[(size_t)v * a.n_points] : 1.0; }
};

// Views of `used` (bit v) in ascending order.
template <int KIND>
__device__ inline void evaluate(const View<KIND>& vw, unsigned used, const double* X, Normal& o) {
  o.cost = 0.0;
  o.h = Sym3{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  o.g0 = 0.0; o.g1 = 0.0; o.g2 = 0.0;
  o.good = true;
  for (int v = 0; v < vw.a.max_views; ++v) {
    if (!((used >> v) & 1u)) continue;
    const double* w = vw.window(v);
    const double wv = vw.weight(v);
    double win[2], ez, jx[3], jy[3];
    project_jac<KIND>(vw.cam(v), X, win, ez, jx, jy);
    const double r0 = win[0] - w[0], r1 = win[1] - w[1];
    if (KIND == PROJECT_PINHOLE && !(ez >= TRI_NEAR_Z)) o.good = false;
    o.cost = o.cost + wv * (r0 * r0 + r1 * r1);
    o.h.a00 = o.h.a00 + wv * (jx[0] * jx[0] + jy[0] * jy[0]);
    o.h.a10 = o.h.a10 + wv * (jx[1] * jx[0] + jy[1] * jy[0]);
    o.h.a11 = o.h.a11 + wv * (jx[1] * jx[1] + jy[1] * jy[1]);
    o.h.a20 = o.h.a20 + wv * (jx[2] * jx[0] + jy[2] * jy[0]);
    o.h.a21 = o.h.a21 + wv * (jx[2] * jx[1] + jy[2] * jy[1]);
    o.h.a22 = o.h.a22 + wv * (jx[2] * jx[2] + jy[2] * jy[2]);
    o.g0 = o.g0 + wv * (jx[0] * r0 + jy[0] * r1);
    o.g1 = o.g1 + wv * (jx[1] * r0 + jy[1] * r1);
    o.g2 = o.g2 + wv * (jx[2] * r0 + jy[2] * r1);
  }
  const double total = o.cost + (fabs(o.h.a00) + fabs(o.h.a10) + fabs(o.h.a11) + fabs(o.h.a20) + fabs(o.h.a21) + fabs(o.h.a22)) +
                       (fabs(o.g0) + fabs(o.g1) + fabs(o.g2));
  if (!finite_d(total)) o.good = false;
}

}  // namespace

// FACTOR: the instantiation behind ut_triangulate_points_info, which also writes the Cholesky factor of H that step 4 forms for
// sigma (a.sqrt_info); everything else is the arithmetic of the other instantiation, in the same order.
template <int KIND, bool FACTOR>
__global__ __launch_bounds__(64) void triangulate_kernel(TriArgs a) {
  const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long long)a.n * a.n_points) return;
  const int i = (int)(idx / a.n_points), p = (int)(idx - (long long)i * a.n_points);
  const int nv = a.max_views;
  const int32_t* rows = a.cam_rows + (size_t)i * nv;
  // ---- index check: a row outside [-1, n_rows) anywhere in the pose and the pose writes nothing
  bool bad_row = false;
  for (int v = 0; v < nv; ++v) bad_row |= rows[v] < -1 || rows[v] >= a.n_rows;
  if (bad_row) {
    if (p == 0) atomicOr(a.status, UT_BAD_SRC_INDEX);
    return;
  }
  const View<KIND> vw{a, rows, a.window + (((size_t)i * nv) * a.n_points + p) * 2,
                      a.weights ? a.weights + ((size_t)i * nv) * a.n_points + p : nullptr};

  // ---- 1. used views, and 2. the start: sum w (I - d d^T) X = sum w (I - d d^T) o
  unsigned used = 0;
  int n_used = 0;
  bool refused = false;
  Sym3 A{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, w_sum = 0.0;
  for (int v = 0; v < nv; ++v) {
    if (rows[v] < 0) continue;
    const double wv = vw.weight(v);
    if (!(finite_d(wv) && wv >= 0.0)) { refused = true; continue; }
    if (!(wv > 0.0)) continue;                      // weight 0: the window is not read
    const double* w = vw.window(v);
    const double wxy[2] = {w[0], w[1]};
    if (!(finite_d(wxy[0]) && finite_d(wxy[1]))) { refused = true; continue; }
    double d[3];
    const double* o = start_ray<KIND>(vw.cam(v), wxy, d);
    if (!(finite_d(d[0]) && finite_d(d[1]) && finite_d(d[2]))) continue;
    used |= 1u << v;
    ++n_used;
    w_sum = w_sum + wv;
    const double dt = d[0] * o[0] + d[1] * o[1] + d[2] * o[2];
    A.a00 = A.a00 + wv * (1.0 - d[0] * d[0]);
    A.a10 = A.a10 + wv * (0.0 - d[1] * d[0]);
    A.a11 = A.a11 + wv * (1.0 - d[1] * d[1]);
    A.a20 = A.a20 + wv * (0.0 - d[2] * d[0]);
    A.a21 = A.a21 + wv * (0.0 - d[2] * d[1]);
    A.a22 = A.a22 + wv * (1.0 - d[2] * d[2]);
    b0 = b0 + wv * (o[0] - d[0] * dt);
    b1 = b1 + wv * (o[1] - d[1] * dt);
    b2 = b2 + wv * (o[2] - d[2] * dt);
  }
  if (n_used < 2) refused = true;

  double X[3] = {0.0, 0.0, 0.0};
  Normal cur;
  cur.cost = 0.0;
  cur.h = Sym3{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  cur.g0 = 0.0; cur.g1 = 0.0; cur.g2 = 0.0;
  cur.good = false;
  int status = refused ? TRI_REFUSED : 0;
  if (!refused) {
    Sym3 l;
    const bool ok = chol3(A, TRI_PIVOT_FRACTION * fmax(A.a00, fmax(A.a11, A.a22)), l);
    if (ok) {
      chol3_solve(l, b0, b1, b2, X);
      evaluate<KIND>(vw, used, X, cur);
    }
    if (!(ok && cur.good)) status = TRI_DEGENERATE;
  }
  const bool live = status == 0;

  // ---- 3. Levenberg-Marquardt: one solve and one evaluation (at the trial) per iteration
  if (live) {
    double lambda = TRI_LAMBDA_START;
    bool done = false;
    for (int it = 0; it < a.max_iters && !done; ++it) {
      const Sym3 damped{cur.h.a00 + lambda * cur.h.a00, cur.h.a10, cur.h.a11 + lambda * cur.h.a11,
                        cur.h.a20, cur.h.a21, cur.h.a22 + lambda * cur.h.a22};
      Sym3 l;
      bool solved = chol3(damped, 0.0, l);
      double step[3];
      chol3_solve(l, -cur.g0, -cur.g1, -cur.g2, step);
      solved = solved && finite_d(step[0]) && finite_d(step[1]) && finite_d(step[2]);
      if (!solved) { step[0] = 0.0; step[1] = 0.0; step[2] = 0.0; }
      const double T[3] = {X[0] + step[0], X[1] + step[1], X[2] + step[2]};
      Normal trial;
      evaluate<KIND>(vw, used, T, trial);
      const bool good = trial.good && solved;
      const double step2 = (step[0] * step[0] + step[1] * step[1]) + step[2] * step[2];
      const double x2 = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
      const bool small = good && step2 <= TRI_STEP_TOL * TRI_STEP_TOL * (1.0 + x2) && lambda <= TRI_LAMBDA_CONVERGED_MAX;
      const bool accept = good && trial.cost < cur.cost;
      const bool stationary = good && !accept && fabs(sqrt(trial.cost / w_sum) - sqrt(cur.cost / w_sum)) <= TRI_FLAT_TOL_PX;
      if (accept) {
        X[0] = T[0]; X[1] = T[1]; X[2] = T[2];
        cur = trial;
        lambda = fmax(lambda * TRI_LAMBDA_DOWN, TRI_LAMBDA_MIN);
      } else {
        lambda = lambda * TRI_LAMBDA_UP;
      }
      done = small || stationary;
    }
    status = done ? TRI_CONVERGED : TRI_AT_MAX_ITERS;
  }

  // ---- 4. uncertainty and outputs; a refused or degenerate point is (0, 0, 0) with sigma +inf
  if (!live) { X[0] = 0.0; X[1] = 0.0; X[2] = 0.0; }
  if (a.points) {
    double* o = a.points + (size_t)idx * 3;
    o[0] = X[0]; o[1] = X[1]; o[2] = X[2];
  }
  if (a.points_f32) {
    float* o = a.points_f32 + (size_t)i * a.point_stride + 3 * p;
    o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
  }
  if (a.info || FACTOR) {
    double sigma = INFINITY, rms = 0.0;
    Sym3 l{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
      if (chol3(cur.h, 0.0, l)) sigma = sqrt(chol3_trace_inverse(l));
      rms = sqrt(cur.cost / w_sum);
    }
    if (a.info) {
      float* o = a.info + (size_t)idx * 4;
      o[0] = (float)rms; o[1] = (float)sigma; o[2] = (float)n_used; o[3] = (float)status;
    }
    if (FACTOR) {                       // 0 where the reported sigma is +inf: the point carries no information
      const bool known = (float)sigma <= 3.0e38f;
      float* o = a.sqrt_info + (size_t)idx * 6;
      o[0] = known ? (float)l.a00 : 0.f; o[1] = known ? (float)l.a10 : 0.f; o[2] = known ? (float)l.a11 : 0.f;
      o[3] = known ? (float)l.a20 : 0.f; o[4] = known ? (float)l.a21 : 0.f; o[5] = known ? (float)l.a22 : 0.f;
    }
  }
  if (a.residual) {
    for (int v = 0; v < nv; ++v) {
      double dist = 0.0;
      if (live && ((used >> v) & 1u)) {
        const double* w = vw.window(v);
        double win[2], ez, jx[3], jy[3];
        project_jac<KIND>(vw.cam(v), X, win, ez, jx, jy);
        const double r0 = win[0] - w[0], r1 = win[1] - w[1];
        dist = sqrt(r0 * r0 + r1 * r1);
      }
      a.residual[((size_t)i * nv + v) * a.n_points + p] = (float)dist;
    }
  }
}

hipError_t launch_triangulate(const TriArgs& a, hipStream_t s) {
  const long long total = (long long)a.n * a.n_points;
  if (total <= 0) return hipSuccess;
  if (a.max_views < 1 || a.max_views > TRI_MAX_VIEWS || total > (1ll << 36)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 63) / 64)), block(64);
  const bool fisheye = a.kind == PROJECT_FISHEYE62;
  if (a.sqrt_info) {
    if (fisheye) hipLaunchKernelGGL((triangulate_kernel<PROJECT_FISHEYE62, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((triangulate_kernel<PROJECT_PINHOLE, true>), grid, block, 0, s, a);
  } else {
    if (fisheye) hipLaunchKernelGGL((triangulate_kernel<PROJECT_FISHEYE62, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((triangulate_kernel<PROJECT_PINHOLE, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace ut
