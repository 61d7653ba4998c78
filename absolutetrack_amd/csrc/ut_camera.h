// fp64 camera arithmetic shared by cropgen.hip (visibility gate, window keypoints), render.hip (ut_project_points),
// triangulate.hip (ut_triangulate_points) and fit_views.hip (ut_fit_pose_views): world -> eye, the forward Fisheye62 projection
// and the reference's unprojection through a cam_params row (layout of ut_warp_crops); one view's projection with its analytic
// Jacobian and the 3 x 3 Cholesky helpers.  Whether the compiler may contract a * b + c follows the translation unit that
// includes this header: cropgen.hip and fit_views.hip keep the default, render.hip and triangulate.hip turn contraction off at
// file scope before the include so that every step rounds like numpy; window_to_world_d turns it off for itself.
#pragma once
#include <hip/hip_runtime.h>

#include "ut_kernels.h"

namespace ut {

// world -> eye of a camera given as cam_params row (R at [12..20], t at [21..23] of camera_to_world)
__device__ inline void world_to_eye_d(const double* cam, const double* w, double* e) {
  const double* r = cam + 12;
  const double* t = cam + 21;
  const double dx = w[0] - t[0], dy = w[1] - t[1], dz = w[2] - t[2];
  e[0] = r[0] * dx + r[3] * dy + r[6] * dz;
  e[1] = r[1] * dx + r[4] * dy + r[7] * dz;
  e[2] = r[2] * dx + r[5] * dy + r[8] * dz;
}

// Fisheye62 eye -> window (lib/common/camera.py:80-85,122-143,308-312)
__device__ inline void fisheye_project_d(const double* cam, const double* e, double* win) {
  const double r = sqrt(e[0] * e[0] + e[1] * e[1]);
  const double sc = atan2(r, e[2]) / fmax(r, 2.938735877055719e-39);
  const double ux = e[0] * sc, uy = e[1] * sc;
  const double k1 = cam[4], k2 = cam[5], k3 = cam[6], k4 = cam[7], p1 = cam[8], p2 = cam[9], k5 = cam[10], k6 = cam[11];
  const double pi2 = 9.869604401089358;
  const double r2 = fmin(fmax(ux * ux + uy * uy, -pi2), pi2);
  const double r4 = r2 * r2, r6 = r2 * r4;
  const double radial = 1 + k1 * r2 + k2 * r4 + k3 * r6 + k4 * (r4 * r4) + k5 * (r4 * r6) + k6 * (r6 * r6);
  const double x = ux * radial, y = uy * radial;
  const double x2 = x * x, y2 = y * y, xy = x * y, rr = x2 + y2;
  win[0] = (x + (2 * p2 * xy + p1 * (rr + 2 * x2))) * cam[0] + cam[2];
  win[1] = (y + (2 * p1 * xy + p2 * (rr + 2 * y2))) * cam[1] + cam[3];
}

// window px -> world point through a cam_params row (Fisheye62CameraModel.window_to_eye, then eye_to_world)
__device__ inline void window_to_world_d(const double* cam, const double* w, double* out) {
#pragma clang fp contract(off)
  const double qx = (w[0] - cam[2]) / cam[0], qy = (w[1] - cam[3]) / cam[1];
  const double k1 = cam[4], k2 = cam[5], k3 = cam[6], k4 = cam[7], k5 = cam[10], k6 = cam[11];
  double x = qx, y = qy;
  for (int it = 0; it < 5; ++it) {          // camera.py:167-179
    const double r2 = x * x + y * y;
    const double rad = 1 + k1 * r2 + k2 * (r2 * r2) + k3 * pow(r2, 3.0) + k4 * pow(r2, 4.0) + k5 * pow(r2, 5.0) +
                       k6 * pow(r2, 6.0);
    x = qx / rad;
    y = qy / rad;
  }
  const double r = sqrt(x * x + y * y);
  const double xs = r / 3.141592653589793;                      // np.sinc(r / pi) = sin(y) / y, y = pi * x
  const double ys = 3.141592653589793 * (xs == 0.0 ? 1.0e-20 : xs);
  const double s = sin(ys) / ys;
  const double e[3] = {x * s, y * s, cos(r)};
  const double* rc = cam + 12;
  const double* tc = cam + 21;
  for (int i = 0; i < 3; ++i) out[i] = (rc[3 * i] * e[0] + rc[3 * i + 1] * e[1] + rc[3 * i + 2] * e[2]) + tc[i];
}

// ---- what triangulate.hip and fit_views.hip share: the 3 x 3 Cholesky helpers and one view's projection with its Jacobian
constexpr double TRI_PIVOT_FRACTION = 1e-10;
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

// The semidefinite variant: a pivot at or below `floor` zeroes its column of L and its entry of rho, where L rho = b by the
// same forward substitution.  One view of a point gives rank 2: that is the normal case, not an error.  L L^T is then `a`
// without the direction the views say nothing about, and L rho = b in every row when b lies in a's range.
__device__ inline void chol3_semidefinite(const Sym3& a, double floor, double b0, double b1, double b2, Sym3& l, double* rho) {
  const bool k0 = a.a00 > floor;
  l.a00 = k0 ? sqrt(a.a00) : 0.0;
  l.a10 = k0 ? a.a10 / l.a00 : 0.0;
  l.a20 = k0 ? a.a20 / l.a00 : 0.0;
  rho[0] = k0 ? b0 / l.a00 : 0.0;
  const double p1 = a.a11 - l.a10 * l.a10;
  const bool k1 = p1 > floor;
  l.a11 = k1 ? sqrt(p1) : 0.0;
  l.a21 = k1 ? (a.a21 - l.a20 * l.a10) / l.a11 : 0.0;
  rho[1] = k1 ? (b1 - l.a10 * rho[0]) / l.a11 : 0.0;
  const double p2 = (a.a22 - l.a20 * l.a20) - l.a21 * l.a21;
  const bool k2 = p2 > floor;
  l.a22 = k2 ? sqrt(p2) : 0.0;
  rho[2] = k2 ? ((b2 - l.a20 * rho[0]) - l.a21 * rho[1]) / l.a22 : 0.0;
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

// The forward half alone: window and eye z.
template <int KIND>
__device__ inline void project_window(const double* cam, const double* X, double* win, double& ez) {
  double e[3];
  if (KIND == PROJECT_FISHEYE62) {
    world_to_eye_d(cam, X, e);
    fisheye_project_d(cam, e, win);
  } else {
    const double* r = cam + 4;
    const double d0 = X[0] - cam[13], d1 = X[1] - cam[14], d2 = X[2] - cam[15];
    e[0] = r[0] * d0 + r[3] * d1 + r[6] * d2;
    e[1] = r[1] * d0 + r[4] * d1 + r[7] * d2;
    e[2] = r[2] * d0 + r[5] * d1 + r[8] * d2;
    win[0] = e[0] / e[2] * cam[0] + cam[2];
    win[1] = e[1] / e[2] * cam[1] + cam[3];
  }
  ez = e[2];
}

}  // namespace ut
