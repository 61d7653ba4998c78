// The cost of the pose fits on 2-D keypoints in camera views, written once: fit_views.hip (ut_fit_pose_views, squared) and
// fit_views_robust.hip (ut_fit_pose_views_robust, Huber and Geman-McClure) instantiate it in ut_fit_dev.h's fit_pose(), and
// fit_views_scale.hip derives it on 27 parameters.  fit_views.hip's header comment: the reduction to 63 rows, the region, registers.
//
// The loss is a compile-time parameter.  The cost is sum_v sum_l w_vl c^2 rho(d_vl^2 / c^2), d the reprojection distance and c
// a scale, both in px:
//   FITV_LOSS_SQUARED          rho(s) = s                                     psi = rho' = 1
//   FITV_LOSS_HUBER            rho(s) = s (s <= 1), 2 sqrt(s) - 1 (s > 1)     psi = 1, 1 / sqrt(s)
//   FITV_LOSS_GEMAN_MCCLURE    rho(s) = s / (1 + s)                           psi = 1 / (1 + s)^2
// The linearisation is iteratively reweighted least squares: finish_rows forms M and b with w_v psi_v where the squared cost
// has w_v, psi_v in fp64 from the residual it already holds.  b is then half the exact gradient of the robust cost; there is no
// second-order (Triggs) term.  The cost hook returns the robust cost itself, so fit_pose()'s accept / reject, lambda and stop
// rules act on it unchanged; `worst` stays the largest raw reprojection distance.  With FITV_LOSS_SQUARED every factor is the
// constant 1 and fit_views.hip compiles to what it compiled to before the loss was a parameter.
// The four kernels in the views repeat their cam_rows index check (the bad_row loop, the atomicOr) on purpose: a shared __device__
// helper, with or without the atomicOr, changes the register allocation of all four files, which sit at the register limit.
#pragma once
#include "ut_camera.h"
#include "ut_fit_dev.h"

namespace ut {

constexpr int FITV_P = 4;        // poses (waves) per workgroup

struct FitViewsLds {             // one wave's region, 15064 bytes: FITV_P of them stay inside the 64 KB a workgroup gets
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
  float target[21][3], w[21];    // 0 (no 3-D targets) and scalar weights sum_v w_vl, 0 = unused
};
static_assert(sizeof(FitViewsLds) == 15064 && sizeof(FitViewsLds) * FITV_P <= 65536, "a workgroup's static LDS");

// psi(d2 / c^2) and c^2 rho(d2 / c^2) of a squared reprojection distance d2, inv_c2 = 1 / c^2.  A d2 that is not finite gives a
// cost that is not finite (Huber: inf x 0, Geman-McClure: inf / inf), which the cost hook turns into +inf.
template <int LOSS>
__device__ inline double fitv_psi(double d2, double inv_c2) {
  if (LOSS == FITV_LOSS_SQUARED) return 1.0;
  const double s = d2 * inv_c2;
  if (LOSS == FITV_LOSS_HUBER) return fmin(1.0, rsqrt(s));
  return 1.0 / ((1.0 + s) * (1.0 + s));
}
template <int LOSS>
__device__ inline double fitv_rho(double d2, double c2, double inv_c2) {
  if (LOSS == FITV_LOSS_SQUARED) return d2;
  const double s = d2 * inv_c2;
  if (LOSS == FITV_LOSS_HUBER) return s <= 1.0 ? d2 : 2.0 * d2 * rsqrt(s) - c2;      // c^2 (2 sqrt(s) - 1)
  return d2 / (1.0 + s);
}

// REGION, PARAMS, STRIDE: the problem's P::Lds, P::NP, P::LD - fit_views.hip's and fit_views_robust.hip's, or FitScaleLds, 27, 29.
template <int KIND, int LOSS = FITV_LOSS_SQUARED, class REGION = FitViewsLds, int PARAMS = 26, int STRIDE = 27>
struct FitViewsCost {
  using Lds = REGION;
  static constexpr int NP = PARAMS, LD = STRIDE;
  static constexpr bool PIVOT_FROM_START = true;
  static constexpr int ROW = KIND == PROJECT_FISHEYE62 ? 32 : 24;
  const FitViewsArgs& a;
  const int32_t* rows = nullptr;  // the pose's cam_rows
  const double* win = nullptr;    // lanes 0..20: the landmark's window in view 0; + v * 42
  const float* wgt = nullptr;     // lanes 0..20: its weight in view 0, or null; + v * 21
  unsigned mask = 0;              // lanes 0..20: bit v = the observation in view v is used
  float worst = 0.f, worst_t = 0.f;      // wave uniform: the largest reprojection distance of the accepted / last evaluated state
  bool started = false;
  double c2 = 1.0, inv_c2 = 1.0;  // the loss's scale squared in px^2 and its inverse: not read by FITV_LOSS_SQUARED
  float* inlier = nullptr;        // [n,max_views,21] or null: psi of every used observation at the returned pose

  __device__ inline const double* cam(int v) const { return a.table + (size_t)rows[v] * ROW; }
  __device__ inline double weight(int v) const { return wgt ? (double)wgt[v * 21] : 1.0; }

  // A landmark's observations, views ascending: used when the view's row is >= 0, the weight finite and > 0 and the window
  // finite; false for a negative or non-finite weight of a seen view and for a non-finite window at a positive weight.  The
  // window of a weight-0 observation is not read.
  __device__ inline bool load(Lds&, int i, int, int lane, float& wl, bool& used) {
    rows = a.cam_rows + (size_t)i * a.max_views;
    if (lane >= 21) return true;
    win = a.window + ((size_t)i * a.max_views * 21 + lane) * 2;
    wgt = a.weights ? a.weights + (size_t)i * a.max_views * 21 + lane : nullptr;
    bool bad = false;
    for (int v = 0; v < a.max_views; ++v) {
      if (rows[v] < 0) continue;
      const float w = wgt ? wgt[v * 21] : 1.f;
      if (!(w >= 0.f && w <= 3.0e38f)) { bad = true; continue; }
      if (!(w > 0.f)) continue;
      const double ux = win[v * 42], uy = win[v * 42 + 1];
      if (!(finite_d(ux) && finite_d(uy))) { bad = true; continue; }
      mask |= 1u << v;
      wl += w;
    }
    used = mask != 0;
    return !bad && wl <= 3.0e38f;
  }
  __device__ inline float row_scale(const Lds&, int) { return 1.f; }

  // rows <- L^T rows and the residual column <- rho, with M = L L^T and L rho = b of this landmark's views at (px, py, pz),
  // every view weighted by w_v psi_v: this lane wrote the rows, nobody else reads them before the wave_sync that follows
  __device__ inline void finish_rows(Lds&, int, float* row, float, float px, float py, float pz) {
    const double X[3] = {px, py, pz};
    Sym3 m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int v = 0; v < a.max_views; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const double w = weight(v);
      double w2[2], ez, jx[3], jy[3];
      project_jac<KIND>(cam(v), X, w2, ez, jx, jy);
      const double r0 = w2[0] - win[v * 42], r1 = w2[1] - win[v * 42 + 1];
      const double wv = LOSS == FITV_LOSS_SQUARED ? w : w * fitv_psi<LOSS>(r0 * r0 + r1 * r1, inv_c2);
      m.a00 += wv * (jx[0] * jx[0] + jy[0] * jy[0]);
      m.a10 += wv * (jx[1] * jx[0] + jy[1] * jy[0]);
      m.a11 += wv * (jx[1] * jx[1] + jy[1] * jy[1]);
      m.a20 += wv * (jx[2] * jx[0] + jy[2] * jy[0]);
      m.a21 += wv * (jx[2] * jx[1] + jy[2] * jy[1]);
      m.a22 += wv * (jx[2] * jx[2] + jy[2] * jy[2]);
      b0 += wv * (jx[0] * r0 + jy[0] * r1);
      b1 += wv * (jx[1] * r0 + jy[1] * r1);
      b2 += wv * (jx[2] * r0 + jy[2] * r1);
    }
    Sym3 l;
    double rho[3];
    chol3_semidefinite(m, TRI_PIVOT_FRACTION * fmax(m.a00, fmax(m.a11, m.a22)), b0, b1, b2, l, rho);
    const float l00 = (float)l.a00, l10 = (float)l.a10, l11 = (float)l.a11, l20 = (float)l.a20, l21 = (float)l.a21,
                l22 = (float)l.a22;
    for (int c = 0; c < NP; ++c) {
      const float a0 = row[c], a1 = row[LD + c], a2 = row[2 * LD + c];
      row[c] = l00 * a0 + l10 * a1 + l20 * a2;
      row[LD + c] = l11 * a1 + l21 * a2;
      row[2 * LD + c] = l22 * a2;
    }
    row[NP] = (float)rho[0]; row[LD + NP] = (float)rho[1]; row[2 * LD + NP] = (float)rho[2];
  }

  // The cost of the state fit_eval left in S.p, +inf when a used observation cannot be projected; the largest reprojection
  // distance goes to worst_t (and to worst for the start, the first state evaluated).
  __device__ inline float cost(const Lds& S, int lane, bool used, float) {
    float c = 0.f, far = 0.f;
    if (used) {
      const double X[3] = {S.p[lane][0], S.p[lane][1], S.p[lane][2]};
      double sum = 0.0, d2max = 0.0;
      bool good = true;
      for (int v = 0; v < a.max_views; ++v) {
        if (!((mask >> v) & 1u)) continue;
        double w2[2], ez;
        project_window<KIND>(cam(v), X, w2, ez);
        const double r0 = w2[0] - win[v * 42], r1 = w2[1] - win[v * 42 + 1];
        const double d2 = r0 * r0 + r1 * r1;
        if (KIND == PROJECT_PINHOLE && !(ez >= TRI_NEAR_Z)) good = false;
        sum += weight(v) * fitv_rho<LOSS>(d2, c2, inv_c2);
        d2max = fmax(d2max, d2);
      }
      good = good && finite_d(sum);
      c = good ? (float)sum : INFINITY;
      far = good ? (float)d2max : 0.f;
    }
    worst_t = sqrtf(wave_max(far));
    if (!started) { worst = worst_t; started = true; }
    return wave_sum(c);
  }
  __device__ inline bool trial(Lds&, int, float) { return true; }
  __device__ inline void keep() { worst = worst_t; }

  // info: rms = sqrt(cost / sum of the used weights) - px at unit weights and residuals below the scale -, the largest
  // reprojection distance of a used observation, iterations, status; residual: the reprojection distance of every used
  // observation at the returned pose; inlier: its psi, from the same residual
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    if (a.info && lane == 0) {
      FitState s = st;
      s.worst = worst;
      fit_store_info(a.info + (size_t)i * 4, s, st.wsum, st.status);
    }
    report_observations(S, i, lane, st);
  }
  // report's `residual` and `inlier`; needs the region's model to be the returned state's
  __device__ inline void report_observations(Lds& S, int i, int lane, const FitState& st) {
    if (!a.residual && !inlier) return;
    if (!st.refused) {                 // S.p holds the last trial: the landmarks of the returned pose once more
      float unused;
      fit_eval(S, S.ang, S.wrist, lane, unused);
    }
    if (lane < 21) {
      const double X[3] = {S.p[lane][0], S.p[lane][1], S.p[lane][2]};
      float* o = a.residual + (size_t)i * a.max_views * 21 + lane;
      float* q = inlier + (size_t)i * a.max_views * 21 + lane;
      for (int v = 0; v < a.max_views; ++v) {
        float dist = 0.f, psi = 0.f;
        if (!st.refused && ((mask >> v) & 1u)) {
          double w2[2], ez;
          project_window<KIND>(cam(v), X, w2, ez);
          const double r0 = w2[0] - win[v * 42], r1 = w2[1] - win[v * 42 + 1];
          dist = (float)sqrt(r0 * r0 + r1 * r1);
          psi = (float)fitv_psi<LOSS>(r0 * r0 + r1 * r1, inv_c2);
        }
        if (!inlier || a.residual) o[v * 21] = dist;      // without `inlier` the early return has seen to a.residual
        if (inlier) q[v * 21] = psi;
      }
    }
  }
};

}  // namespace ut
