// The information of a pose under the cost of the fits in the views: ut_pose_information_views (include/umetrack_hip_uncertainty.h).
// One linearisation of ut_fit_views_dev.h's cost at the pose as given - fit_load, fit_eval, fit_pivot and fit_linearise of
// ut_fit_dev.h - then H = J^T J (+ the prior) out of S.a, its Cholesky factor, and through the factor sqrt(diag H^-1)
// and G_l H^-1 G_l^T of the 21 landmarks.  Nothing is fitted and nothing of the pose is written.  The yardstick is the float64
// restatement in tests/uncertainty_cases.py.
//
// The fit's region (FitViewsLds, four poses per workgroup, one wave per pose, no workgroup barrier, wave-uniform branches):
//  (1) H: fit_linearise on FitViewsCost<KIND, LOSS> leaves the reduced rows in S.jl and H in S.a.  Lanes 0..19 add 1 / sigma^2
//      to their diagonal entry, the 351 entries go out.
//  (2) factor: lane i keeps row i of D^-1/2 H D^-1/2 (D = diag H, unit diagonal: plain condition 4e5, scaled <= 800) in
//      registers, the right-looking factorisation of fit_solve with the smallest pivot tracked; a pivot <= COV_MIN_PIVOT ends it
//      (COV_SINGULAR).  The rows stay in registers over (3).
//  (3) G again: finish_rows overwrote the landmarks' raw Jacobian rows, and unused landmarks never had any.  fit_rows - the first
//      half of fit_linearise - once more with a problem that marks all 21 landmarks used and finishes nothing: S.jl = G [63][27],
//      the rows of (1) by construction.
//  (4) L' = D^1/2 L, the factor of H itself, into S.a (1 / L'_ii on the diagonal).  Lane r < 63 solves L' y = G_r forward with y in
//      registers - the factor is read at wave-uniform addresses, a broadcast - and leaves y in its own row of S.jl; lane l < 21
//      then forms the six sums of Sigma_l = Y_l^T Y_l over rows 3 l .. 3 l + 2 (row stride 27 x 3 = 81 words, odd: no bank
//      conflict).  Lane i < 26 solves L' y = e_i the same way: (H^-1)_ii = |y|^2.
// Registers and scratch: DESIGN.md, "Uncertainty of a pose fitted in the views".
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

constexpr int COV_NP = 26, COV_LD = 27;

// fit_rows' rows as they are before finish_rows, of every landmark: the world Jacobian G [63][26] at row scale 1.
struct RawRows {
  using Lds = FitViewsLds;
  static constexpr int NP = COV_NP, LD = COV_LD;
  __device__ inline float row_scale(const Lds&, int) { return 1.f; }
  __device__ inline void finish_rows(Lds&, int, float*, float, float, float, float) {}
};

// Row `lane` of D^-1/2 A D^-1/2 into a[] (A the leading 26 x 26 block of S.a, D its diagonal) and its factorisation in place,
// fit_solve's: a[k] = L_lane,k for k <= lane afterwards.  sd = sqrt(D_lane) on lane < 26.  min_pivot: the smallest pivot (the
// diagonal of the Schur complement) up to and including the one that ended the factorisation; false when a diagonal entry of A is
// not positive and finite (pivot 0) or a pivot is <= COV_MIN_PIVOT.
__device__ inline bool cov_factor(const FitViewsLds& S, int lane, float (&a)[COV_NP], float& sd, float& min_pivot) {
  constexpr int NP = COV_NP;
  const bool row = lane < NP;
  const float d = row ? S.a[lane][lane] : 1.f;
  const bool has = d > 0.f && d <= 3.0e38f;
  sd = has ? sqrtf(d) : 0.f;
  const float s = has ? 1.f / sd : 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const float sk = lane_value(s, k);
    a[k] = (row && k < lane) ? S.a[row ? lane : 0][k] * s * sk : ((row && k == lane && has) ? 1.f : 0.f);
  }
  min_pivot = 1.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float piv = lane_value(a[j], j);
    const bool good = piv > COV_MIN_PIVOT && piv <= 3.0e38f;
    min_pivot = fminf(min_pivot, good ? piv : fmaxf(piv, 0.f));      // fmaxf drops a NaN: 0
    if (!good) return false;
    const float inv = 1.f / sqrtf(piv);
    a[j] *= inv;
#pragma unroll
    for (int k = j + 1; k < NP; ++k) a[k] = fmaf(-a[j], lane_value(a[j], k), a[k]);
  }
  return true;
}

// y = L'^-1 b, L' in S.a (strictly lower entries, 1 / L'_jj on the diagonal): every lane its own b and y, the factor broadcast.
__device__ inline void cov_forward(const FitViewsLds& S, const float (&b)[COV_NP], float (&y)[COV_NP]) {
#pragma unroll
  for (int j = 0; j < COV_NP; ++j) {
    float t = b[j];
#pragma unroll
    for (int k = 0; k < j; ++k) t = fmaf(-S.a[j][k], y[k], t);
    y[j] = t * S.a[j][j];
  }
}

template <int KIND, int LOSS>
__global__ __launch_bounds__(64 * FITV_P, 2) void pose_information_views_kernel(const PoseInfoViewsArgs a) {
  __shared__ FitViewsLds s_all[FITV_P];
  const FitViewsArgs& g = a.robust.views;
  const int i = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  if (i >= g.pose.n) return;                          // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  // index check, as in fit_pose_views_kernel: a row outside [-1, n_rows) anywhere in the pose and the pose writes nothing
  bool bad_row = false;
  for (int v = 0; v < g.max_views; ++v) {
    const int r = g.cam_rows[(size_t)i * g.max_views + v];
    bad_row |= r < -1 || r >= g.n_rows;
  }
  if (bad_row) {
    if (lane == 0) atomicOr(g.status, UT_BAD_SRC_INDEX);
    return;
  }
  FitViewsLds& S = s_all[threadIdx.x >> 6];
  FitViewsCost<KIND, LOSS> prob{g};
  prob.c2 = (double)a.robust.loss_scale * (double)a.robust.loss_scale;
  prob.inv_c2 = 1.0 / prob.c2;

  FitState st;
  fit_load(prob, S, g.pose, i, lane, st);
  float prior = 0.f;                                  // lanes 0..19: 1 / sigma^2
  if (a.angle_sigma) {
    const float sg = lane < 20 ? a.angle_sigma[(size_t)(g.pose.n_models == 1 ? 0 : i) * 20 + lane] : 1.f;
    prior = lane < 20 ? 1.f / (sg * sg) : 0.f;
    if (wave_any(!(sg > 0.f) || !(sg <= 3.0e38f) || !(prior <= 3.0e38f))) st.refused = true;      // 1 / sigma^2 must be finite too
  }
  if (!st.refused) {
    const float iso = fit_eval(S, S.ang, S.wrist, lane, st.worst);
    fit_pivot(S.p, lane, st);
    st.cost = prob.cost(S, lane, st.used, iso);
    if (!(st.cost <= 3.0e38f)) st.refused = true;
  }

  float* o_info = a.pose_info ? a.pose_info + (size_t)i * 351 : nullptr;
  float* o_pivot = a.pivot ? a.pivot + (size_t)i * 3 : nullptr;
  float* o_sigma = a.param_sigma ? a.param_sigma + (size_t)i * 26 : nullptr;
  float* o_cov = a.landmark_cov ? a.landmark_cov + (size_t)i * 126 : nullptr;
  float* o_stat = a.info ? a.info + (size_t)i * 4 : nullptr;
  if (st.refused) {
    if (o_info) for (int e = lane; e < 351; e += 64) o_info[e] = 0.f;
    if (o_cov) for (int e = lane; e < 126; e += 64) o_cov[e] = 0.f;
    if (o_sigma && lane < 26) o_sigma[lane] = 0.f;
    if (o_pivot && lane < 3) o_pivot[lane] = 0.f;
    if (o_stat && lane < 4) o_stat[lane] = lane == 3 ? (float)COV_REFUSED : 0.f;
    return;
  }

  // (1)
  fit_linearise(prob, S, lane, st);
  if (lane < 20) S.a[lane][lane] += prior;            // the lane's own entry; read again only behind the wave_sync
  wave_sync();
  if (o_info) {
    for (int e = lane; e < 351; e += 64) {
      int r = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
      if (r * (r + 1) / 2 > e) --r;
      if ((r + 1) * (r + 2) / 2 <= e) ++r;
      o_info[e] = S.a[r][e - r * (r + 1) / 2];
    }
  }
  if (o_pivot && lane < 3) o_pivot[lane] = lane == 0 ? st.cx : (lane == 1 ? st.cy : st.cz);

  // (2)
  float L[COV_NP], sd, min_pivot;
  const bool regular = cov_factor(S, lane, L, sd, min_pivot);
  if (!regular) {                                     // wave uniform: pivots are read by v_readlane
    if (o_sigma && lane < 26) o_sigma[lane] = INFINITY;
    if (o_cov) for (int e = lane; e < 126; e += 64) o_cov[e] = (e % 6 == 0 || e % 6 == 2 || e % 6 == 5) ? INFINITY : 0.f;
    if (o_stat && lane < 4)
      o_stat[lane] = lane == 0 ? sqrtf(st.cost / st.wsum) : (lane == 1 ? INFINITY : (lane == 2 ? min_pivot : (float)COV_SINGULAR));
    return;
  }

  // (3)
  if (o_cov || o_stat) {
    RawRows raw;
    FitState all = st;
    all.used = lane < 21;
    fit_rows(raw, S, lane, all);
  }

  // (4)
  if (lane < COV_NP) {
#pragma unroll
    for (int k = 0; k < COV_NP; ++k) {
      if (k < lane) S.a[lane][k] = L[k] * sd;
      else if (k == lane) S.a[lane][k] = 1.f / (L[k] * sd);
    }
  }
  wave_sync();
  float b[COV_NP], y[COV_NP];
  if (o_sigma) {
#pragma unroll
    for (int k = 0; k < COV_NP; ++k) b[k] = k == lane ? 1.f : 0.f;
    cov_forward(S, b, y);
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < COV_NP; ++k) s2 = fmaf(y[k], y[k], s2);
    if (lane < COV_NP) o_sigma[lane] = sqrtf(s2);
  }
  float worst = 0.f;
  if (o_cov || o_stat) {
    float* mine = S.jl + (lane < 63 ? lane : 0) * COV_LD;
#pragma unroll
    for (int k = 0; k < COV_NP; ++k) b[k] = lane < 63 ? mine[k] : 0.f;
    cov_forward(S, b, y);
    if (lane < 63) {
#pragma unroll
      for (int k = 0; k < COV_NP; ++k) mine[k] = y[k];
    }
    wave_sync();
    float trace = 0.f;
    if (lane < 21) {
      const float *yx = S.jl + 3 * lane * COV_LD, *yy = yx + COV_LD, *yz = yy + COV_LD;
      float xx = 0.f, xy = 0.f, yyy = 0.f, zx = 0.f, zy = 0.f, zz = 0.f;
#pragma unroll
      for (int k = 0; k < COV_NP; ++k) {
        const float u = yx[k], v = yy[k], w = yz[k];
        xx = fmaf(u, u, xx); xy = fmaf(v, u, xy); yyy = fmaf(v, v, yyy);
        zx = fmaf(w, u, zx); zy = fmaf(w, v, zy); zz = fmaf(w, w, zz);
      }
      if (o_cov) {
        float* o = o_cov + 6 * lane;
        o[0] = xx; o[1] = xy; o[2] = yyy; o[3] = zx; o[4] = zy; o[5] = zz;
      }
      trace = xx + yyy + zz;
    }
    worst = wave_max(trace);
  }
  if (o_stat && lane < 4)
    o_stat[lane] = lane == 0 ? sqrtf(st.cost / st.wsum) : (lane == 1 ? sqrtf(worst) : (lane == 2 ? min_pivot : (float)COV_OK));
}

template <int KIND>
void launch_kind(const PoseInfoViewsArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  if (a.robust.loss == FITV_LOSS_HUBER)
    hipLaunchKernelGGL((pose_information_views_kernel<KIND, FITV_LOSS_HUBER>), grid, block, 0, s, a);
  else if (a.robust.loss == FITV_LOSS_GEMAN_MCCLURE)
    hipLaunchKernelGGL((pose_information_views_kernel<KIND, FITV_LOSS_GEMAN_MCCLURE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((pose_information_views_kernel<KIND, FITV_LOSS_SQUARED>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_pose_information_views(const PoseInfoViewsArgs& a, hipStream_t s) {
  const FitViewsArgs& g = a.robust.views;
  if (g.pose.n <= 0) return hipSuccess;
  if (g.max_views < 1 || g.max_views > TRI_MAX_VIEWS || a.robust.loss < FITV_LOSS_SQUARED || a.robust.loss > FITV_LOSS_GEMAN_MCCLURE ||
      !g.pose.init_ja || !g.pose.init_xf)
    return hipErrorInvalidValue;
  const dim3 grid((g.pose.n + FITV_P - 1) / FITV_P), block(64 * FITV_P);
  if (g.kind == PROJECT_FISHEYE62) launch_kind<PROJECT_FISHEYE62>(a, grid, block, s);
  else launch_kind<PROJECT_PINHOLE>(a, grid, block, s);
  return hipGetLastError();
}

}  // namespace ut
