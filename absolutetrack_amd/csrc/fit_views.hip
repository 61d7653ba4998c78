// The pose fit on 2-D keypoints in camera views, fp32 solver with an fp64 projection: ut_fit_pose_views
// (include/umetrack_hip_views.h).  The cost is the reprojection error itself, sum_v sum_l w_vl |project_v(landmark_l) - u_vl|^2,
// over every detection of every view through the exact camera model of ut_project_points / ut_triangulate_points - a landmark
// that one camera alone sees counts, and a hand that one camera alone sees can be fitted: its known size fixes its depth.  The
// yardstick is the float64 restatement in tests/views_cases.py.
//
// This is ut_fit_pose_info (fit_info.hip) with the factor derived again at every accepted state and the virtual target moved
// with it.  The solver is ut_fit_dev.h's fit_pose(), on fit.hip's 26 parameters and 63 rows.  At each linearisation the lane of
// landmark l computes, in fp64 with the views in ascending order, M = sum_v w_v J_v^T J_v (3 x 3, positive semidefinite) and
// b = sum_v w_v J_v^T r_v with the analytic 2 x 3 Jacobian J_v of ut_camera.h's project_jac, factors M = L L^T by the
// semidefinite Cholesky of ut_camera.h (a pivot at or below UT_TRI_PIVOT_FRACTION x the largest diagonal entry zeroes its column:
// one view gives rank 2), solves L rho = b, and replaces its three Jacobian rows a by L^T a - as fit_info.hip's finish_rows
// does - and its residual column by rho.  J^T J and J^T r of the 63 rows are then the Gauss-Newton normal equations of the
// stacked 2 x views x 21 reprojection residuals, which would not fit a region.  The cost hook evaluates the true reprojection
// cost of the state fit_eval left in S.p: per landmark in fp64 over ascending views, rounded once, then wave_sum.  A state in
// which a used observation is not finite or lies in front of UT_TRI_NEAR_Z of a used pinhole view costs +inf: a rejected trial,
// or a refused start.  There are no 3-D targets: the wrist increment turns about the weighted centroid of the START's
// landmarks (weight sum_v w_vl), whose extent scales the translation's step tolerance (PIVOT_FROM_START of ut_fit_dev.h).
//
// Windows, weights and camera rows stay in global memory: a lane reads each of its values once per evaluation, a pose's 21
// lanes share its camera rows, and a launch's rows stay in L2.  The region is FitInfoLds without the factors: 4 x 15064 =
// 60256 bytes of the 64 KB a workgroup gets.  The projection is fp64 on the fp32 landmark: project - u is the difference of
// two numbers of some 300 px, where fp32 would lose the cost's digits.  This file keeps the default contraction, like fit.hip.
//
// Registers.  With the fp64 projection inlined and nothing said, the Fisheye62 kernel takes 256 VGPRs and 5 AGPRs - one wave
// per SIMD, where fit_pose_info_kernel's 227 leave room for two workgroups per CU - and 8192 hands take 2.16 x
// ut_fit_pose_info's time.  __launch_bounds__(256, 2) holds it to 254 VGPRs without scratch: 1.44 x.  The projection out of
// line (arguments and results by value) took 193 VGPRs, 80 bytes of scratch per lane for the call frames and 1.29 x, but was
// one iteration over the iteration rule of tests/test_gpu_views.py on 2 of 148 full fits; windows and weights in LDS (three
// poses per workgroup) 1.53 x.  DESIGN.md, "Pose from keypoints in the views", has the table.
#include "ut_camera.h"
#include "ut_fit_dev.h"

namespace ut {
namespace {

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

template <int KIND>
struct FitViewsCost {
  using Lds = FitViewsLds;
  static constexpr int NP = 26, LD = 27;
  static constexpr bool PIVOT_FROM_START = true;
  static constexpr int ROW = KIND == PROJECT_FISHEYE62 ? 32 : 24;
  const FitViewsArgs& a;
  const int32_t* rows = nullptr;  // the pose's cam_rows
  const double* win = nullptr;    // lanes 0..20: the landmark's window in view 0; + v * 42
  const float* wgt = nullptr;     // lanes 0..20: its weight in view 0, or null; + v * 21
  unsigned mask = 0;              // lanes 0..20: bit v = the observation in view v is used
  float worst = 0.f, worst_t = 0.f;      // wave uniform: the largest reprojection distance of the accepted / last evaluated state
  bool started = false;

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

  // rows <- L^T rows and the residual column <- rho, with M = L L^T and L rho = b of this landmark's views at (px, py, pz):
  // this lane wrote the rows, nobody else reads them before the wave_sync that follows
  __device__ inline void finish_rows(Lds&, int, float* row, float, float px, float py, float pz) {
    const double X[3] = {px, py, pz};
    Sym3 m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int v = 0; v < a.max_views; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const double wv = weight(v);
      double w2[2], ez, jx[3], jy[3];
      project_jac<KIND>(cam(v), X, w2, ez, jx, jy);
      const double r0 = w2[0] - win[v * 42], r1 = w2[1] - win[v * 42 + 1];
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

  // The reprojection cost of the state fit_eval left in S.p, +inf when a used observation cannot be projected; the largest
  // reprojection distance goes to worst_t (and to worst for the start, the first state evaluated).
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
        sum += weight(v) * d2;
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

  // info: rms = sqrt(cost / sum of the used weights) - px at unit weights -, the largest reprojection distance of a used
  // observation, iterations, status; residual: the reprojection distance of every used observation at the returned pose
  __device__ inline void report(Lds& S, int i, int lane, const FitState& st) {
    if (a.info && lane == 0) {
      FitState s = st;
      s.worst = worst;
      fit_store_info(a.info + (size_t)i * 4, s, st.wsum, st.status);
    }
    if (!a.residual) return;
    if (!st.refused) {                 // S.p holds the last trial: the landmarks of the returned pose once more
      float unused;
      fit_eval(S, S.ang, S.wrist, lane, unused);
    }
    if (lane < 21) {
      const double X[3] = {S.p[lane][0], S.p[lane][1], S.p[lane][2]};
      float* o = a.residual + (size_t)i * a.max_views * 21 + lane;
      for (int v = 0; v < a.max_views; ++v) {
        float dist = 0.f;
        if (!st.refused && ((mask >> v) & 1u)) {
          double w2[2], ez;
          project_window<KIND>(cam(v), X, w2, ez);
          const double r0 = w2[0] - win[v * 42], r1 = w2[1] - win[v * 42 + 1];
          dist = (float)sqrt(r0 * r0 + r1 * r1);
        }
        o[v * 21] = dist;
      }
    }
  }
};

template <int KIND>
__global__ __launch_bounds__(64 * FITV_P, 2) void fit_pose_views_kernel(const FitViewsArgs a) {
  __shared__ FitViewsLds s_all[FITV_P];
  const int i = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  if (i >= a.pose.n) return;                          // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  // index check: a row outside [-1, n_rows) anywhere in the pose and the pose writes nothing
  bool bad_row = false;
  for (int v = 0; v < a.max_views; ++v) {
    const int r = a.cam_rows[(size_t)i * a.max_views + v];
    bad_row |= r < -1 || r >= a.n_rows;
  }
  if (bad_row) {
    if (lane == 0) atomicOr(a.status, UT_BAD_SRC_INDEX);
    return;
  }
  FitViewsCost<KIND> cost{a};
  fit_pose(cost, s_all[threadIdx.x >> 6], a.pose, i, lane);
}

}  // namespace

hipError_t launch_fit_pose_views(const FitViewsArgs& a, hipStream_t s) {
  if (a.pose.n <= 0) return hipSuccess;
  if (a.max_views < 1 || a.max_views > TRI_MAX_VIEWS) return hipErrorInvalidValue;
  const dim3 grid((a.pose.n + FITV_P - 1) / FITV_P), block(64 * FITV_P);
  if (a.kind == PROJECT_FISHEYE62) hipLaunchKernelGGL(fit_pose_views_kernel<PROJECT_FISHEYE62>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(fit_pose_views_kernel<PROJECT_PINHOLE>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
