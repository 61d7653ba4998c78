// fp64 camera arithmetic shared by cropgen.hip (visibility gate, window keypoints), render.hip (ut_project_points) and
// triangulate.hip (ut_triangulate_points): world -> eye, the forward Fisheye62 projection and the reference's unprojection
// through a cam_params row (layout of ut_warp_crops).  Whether the compiler may contract a * b + c follows the translation
// unit that includes this header: cropgen.hip keeps the default, render.hip and triangulate.hip turn contraction off at file
// scope before the include so that every step rounds like numpy; window_to_world_d turns it off for itself.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace ut
