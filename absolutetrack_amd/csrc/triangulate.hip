// Points from views (ut_triangulate_points, include/umetrack_hip_triangulate.h; ut_triangulate_points_info,
// include/umetrack_hip_info.h): the inverse of ut_project_points.  Window coordinates of one point in several cameras -> the
// world point, its reprojection residuals and its uncertainty - as one number, or as the factor of its 3 x 3 information.
// One thread per (pose, point); fp64 throughout.  Per thread: a linear start from the views' rays, then Levenberg-Marquardt on
// the reprojection error through the exact forward model (world_to_eye_d + fisheye_project_d of ut_camera.h, or the pinhole of
// render.hip) with an analytic 2 x 3 Jacobian per view.  The views are visited in ascending order by a loop bounded by
// max_views (<= TRI_MAX_VIEWS) that reads each view's camera row, window and weight from global memory every time - a pose's
// 21 points share their camera rows, so these loads hit the cache - and keeps only sums in registers: no per-view private
// array, no LDS, no scratch, no atomics but the index check's status bit.  Every multiply and add of this file rounds on
// its own (no contraction), like the numpy restatement it is tested against (tests/triangulate_cases.py).
#pragma clang fp contract(off)
#include "ut_camera.h"
#include "ut_kernels.h"

namespace ut {

namespace {

constexpr double TRI_PIVOT_FRACTION = 1e-10;
constexpr double TRI_LAMBDA_START = 1e-6, TRI_LAMBDA_DOWN = 0.1, TRI_LAMBDA_UP = 10.0, TRI_LAMBDA_MIN = 1e-12;
constexpr double TRI_LAMBDA_CONVERGED_MAX = 1.0;   // a small step under heavy damping is a stall, not convergence
constexpr double TRI_STEP_TOL = 1e-12;             // x sqrt(1 + |X|^2)
constexpr double TRI_FLAT_TOL_PX = 1e-11;          // rms residual of a rejected trial this close to the accepted one
constexpr double TRI_NEAR_Z = 1e-4;                // near plane of a pinhole view (lib/common/crop.py:25)

__device__ inline bool finite_d(double x) { return fabs(x) <= 1.79769313486231570e308; }      // false for a NaN

// symmetric 3 x 3 in the order a00 a10 a11 a20 a21 a22
struct Sym3 { double a00, a10, a11, a20, a21, a22; };

// Cholesky factor (same layout); false when a pivot is not finite or not above `floor`
__device__ inline bool chol3(const Sym3& a, double floor, Sym3& l) {
  l.a00 = sqrt(a.a00);
  l.a10 = a.a10 / l.a00;
  l.a20 = a.a20 / l.a00;
  const double p1 = a.a11 - l.a10 * l.a10;
  l.a11 = sqrt(p1);
  l.a21 = (a.a21 - l.a20 * l.a10) / l.a11;
  const double p2 = (a.a22 - l.a20 * l.a20) - l.a21 * l.a21;
  l.a22 = sqrt(p2);
  return a.a00 > floor && p1 > floor && p2 > floor && finite_d(a.a00 + p1 + p2);
}

__device__ inline void chol3_solve(const Sym3& l, double b0, double b1, double b2, double* x) {
  const double y0 = b0 / l.a00;
  const double y1 = (b1 - l.a10 * y0) / l.a11;
  const double y2 = ((b2 - l.a20 * y0) - l.a21 * y1) / l.a22;
  x[2] = y2 / l.a22;
  x[1] = (y1 - l.a21 * x[2]) / l.a11;
  x[0] = ((y0 - l.a10 * x[1]) - l.a20 * x[2]) / l.a00;
}

// trace of (L L^T)^-1 = |L^-1|_F^2
__device__ inline double chol3_trace_inverse(const Sym3& l) {
  const double m00 = 1 / l.a00, m11 = 1 / l.a11, m22 = 1 / l.a22;
  const double m10 = -(l.a10 * m00) / l.a11;
  const double m21 = -(l.a21 * m11) / l.a22;
  const double m20 = -(l.a20 * m00 + l.a21 * m10) / l.a22;
  return ((m00 * m00 + m10 * m10) + (m20 * m20 + m11 * m11)) + (m21 * m21 + m22 * m22);
}

// One view of one point: window, eye z and d window / d world point (jx = row of window x, jy = row of window y).
template <int KIND>
__device__ inline void project_jac(const double* cam, const double* X, double* win, double& ez, double* jx, double* jy) {
  double e[3], dx[3], dy[3];      // d win / d eye
  const double* r;
  if (KIND == PROJECT_FISHEYE62) {
    r = cam + 12;
    world_to_eye_d(cam, X, e);
    fisheye_project_d(cam, e, win);
    // the same intermediates once more for the derivative (the compiler shares them): u = theta (ex, ey) / rad_e
    const double rad_e = sqrt(e[0] * e[0] + e[1] * e[1]);
    const double sc = atan2(rad_e, e[2]) / fmax(rad_e, 2.938735877055719e-39);
    const double ux = e[0] * sc, uy = e[1] * sc;
    const double k1 = cam[4], k2 = cam[5], k3 = cam[6], k4 = cam[7], p1 = cam[8], p2 = cam[9], k5 = cam[10], k6 = cam[11];
    const double pi2 = 9.869604401089358;
    const double r2 = fmin(fmax(ux * ux + uy * uy, -pi2), pi2);
    const double r4 = r2 * r2, r6 = r2 * r4;
    const double radial = 1 + k1 * r2 + k2 * r4 + k3 * r6 + k4 * (r4 * r4) + k5 * (r4 * r6) + k6 * (r6 * r6);
    const double x = ux * radial, y = uy * radial;
    // d u / d e
    const double rho2 = rad_e * rad_e + e[2] * e[2];
    const double b = e[2] / rho2;
    const double rs = rad_e * rad_e;
    const bool centre = rs <= 1e-24 * rho2;           // on the optical axis: the limit, d u / d e_xy = I / ez
    const double rs_ = centre ? 1.0 : rs;
    const double cxx = e[0] * e[0] / rs_, cxy = e[0] * e[1] / rs_, cyy = e[1] * e[1] / rs_;
    const double ux_ex = centre ? 1 / e[2] : b * cxx + sc * cyy;
    const double ux_ey = centre ? 0.0 : (b - sc) * cxy;
    const double uy_ey = centre ? 1 / e[2] : b * cyy + sc * cxx;
    const double ux_ez = -e[0] / rho2, uy_ez = -e[1] / rho2;
    // d (x, y) / d u: the radial polynomial
    const double drad = 2 * (k1 + 2 * k2 * r2 + 3 * k3 * r4 + 4 * k4 * r6 + 5 * k5 * (r4 * r4) + 6 * k6 * (r4 * r6));
    const double x_ux = radial + ux * ux * drad, x_uy = ux * uy * drad;
    const double y_ux = x_uy, y_uy = radial + uy * uy * drad;
    // d w / d (x, y): the tangential terms
    const double wx_x = 1 + 2 * p2 * y + 6 * p1 * x, wx_y = 2 * p2 * x + 2 * p1 * y;
    const double wy_x = wx_y, wy_y = 1 + 2 * p1 * x + 6 * p2 * y;
    const double ax = (wx_x * x_ux + wx_y * y_ux) * cam[0], ay = (wx_x * x_uy + wx_y * y_uy) * cam[0];
    const double bx = (wy_x * x_ux + wy_y * y_ux) * cam[1], by = (wy_x * x_uy + wy_y * y_uy) * cam[1];
    dx[0] = ax * ux_ex + ay * ux_ey; dx[1] = ax * ux_ey + ay * uy_ey; dx[2] = ax * ux_ez + ay * uy_ez;
    dy[0] = bx * ux_ex + by * ux_ey; dy[1] = bx * ux_ey + by * uy_ey; dy[2] = bx * ux_ez + by * uy_ez;
  } else {                         // pinhole crop camera: fx fy cx cy | R(9) t(3) of camera_to_world, as render.hip projects
    r = cam + 4;
    const double d0 = X[0] - cam[13], d1 = X[1] - cam[14], d2 = X[2] - cam[15];
    e[0] = r[0] * d0 + r[3] * d1 + r[6] * d2;
    e[1] = r[1] * d0 + r[4] * d1 + r[7] * d2;
    e[2] = r[2] * d0 + r[5] * d1 + r[8] * d2;
    win[0] = e[0] / e[2] * cam[0] + cam[2];
    win[1] = e[1] / e[2] * cam[1] + cam[3];
    dx[0] = cam[0] / e[2]; dx[1] = 0.0; dx[2] = -(cam[0] * e[0]) / (e[2] * e[2]);
    dy[0] = 0.0; dy[1] = cam[1] / e[2]; dy[2] = -(cam[1] * e[1]) / (e[2] * e[2]);
  }
  ez = e[2];
  // d e_i / d X_j = R[j][i]
  jx[0] = dx[0] * r[0] + dx[1] * r[1] + dx[2] * r[2];
  jx[1] = dx[0] * r[3] + dx[1] * r[4] + dx[2] * r[5];
  jx[2] = dx[0] * r[6] + dx[1] * r[7] + dx[2] * r[8];
  jy[0] = dy[0] * r[0] + dy[1] * r[1] + dy[2] * r[2];
  jy[1] = dy[0] * r[3] + dy[1] * r[4] + dy[2] * r[5];
  jy[2] = dy[0] * r[6] + dy[1] * r[7] + dy[2] * r[8];
}

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
