// Starts for the pose fits in the views from the detections alone, and the selection among fitted candidates:
// ut_start_pose_views and ut_select_pose (include/umetrack_hip_start.h).  The yardstick is the float64 restatement in
// tests/start_cases.py.
//
// ut_start_pose_views is generalised PnP by orthogonal iteration: for one bank pose the hand is a rigid set of 21 points p_l, every
// used observation a ray (o_v, d_vl), and sum w |A (R p_l + t - o_v)|^2 with A = I - d d^T is minimised by alternating the closed
// translation t = -(sum w A)^-1 sum w A (R p_l - o_v) with the Kabsch rotation of p_l onto the foot points of R p_l + t on their
// rays.  The iteration has many fixed points - a flat hand seen by one camera looks much alike from the palm and from the back - so
// it runs from a set of rotation seeds, and each end is scored by the exact reprojection cost of ut_fit_pose_views.
//
// One wave per (hand, bank pose), every wave in an LDS region of its own, no workgroup barrier (ut_fit_dev.h's wave_sync).  The
// wave runs the forward function once through ut_fk.h (fit_eval) under the identity wrist and stages cooperatively: the lane of
// landmark l tests its observations by fit_views.hip's rules, unprojects the used ones by triangulate.hip's start ray and appends
// them - views ascending, landmarks ascending within a view, positions by ballot - to a compact list (direction, window, weight,
// view, landmark).  Then ONE LANE PER SEED runs its whole iteration alone: every LDS address in the loop is wave uniform (a
// broadcast, no bank conflict), there is no cross-lane traffic, R, t and the 3 x 3 correlation stay in registers, and the rotation
// is ut_math.h's kabsch_rotation (Jacobi on H^T H with the rank-2 completion: a flat hand is the normal case).  Trip counts are
// `iters` and the number of observations, both wave uniform; only the Jacobi sweeps inside the rotation solve diverge.  fp64
// throughout, as ut_camera.h.  Since sum w (p_l - pc) = 0 for the weighted centroid pc, the correlation is formed in one pass
// as H = sum w (p_l - pc) (R (p_l - pc) - A z)^T with z = R p_l + t - o_v: the foot point minus the constant R pc + t.
// The score: project_window<KIND> of R p_l + t for every observation, summed in list order, +inf if the sum is not finite or a
// used pinhole view has the point in front of TRI_NEAR_Z.  A butterfly argmin over (score, lane) ends the kernel; the winning lane
// writes the wrist and the info row.  This file keeps the default contraction, like fit_views.hip.
//
// The index check is the fourth copy of fit_views.hip's on purpose (ut_fit_views_dev.h says why).
#include "ut_camera.h"
#include "ut_fit_dev.h"

namespace ut {
namespace {

constexpr int STV_P = 4;                          // (hand, bank pose) pairs, i.e. waves, per workgroup
constexpr int STV_OBS = TRI_MAX_VIEWS * 21;

struct StartLds {                 // one wave's region
  float hm[321];                  // the hand's packed model
  float local[20][12], prefix[20][12], frame[17][12];      // fit_eval's
  float p[21][3];                 // landmarks of the bank pose under the identity wrist (mirrored: column 0 negated)
  float target[21][3], w[21];     // fit_eval's: 0
  float ang[20], wrist[12];
  int rows[TRI_MAX_VIEWS];        // the hand's cam_rows
  double pl[21][3];               // p in fp64
  double org[TRI_MAX_VIEWS][3];   // camera centres
  double d[STV_OBS][3], win[STV_OBS][2], wt[STV_OBS];      // the used observations: unit direction, window, weight
  unsigned char view[STV_OBS], lm[STV_OBS];
};
static_assert(sizeof(StartLds) * STV_P <= 65536, "a workgroup's static LDS");

// triangulate.hip's start ray: the unit direction of a window point in the world; the origin is the camera centre (returned).
template <int KIND>
__device__ inline const double* start_ray(const double* cam, const double* w, double* d) {
  const double* t;
  if (KIND == PROJECT_FISHEYE62) {
    double p[3];
    window_to_world_d(cam, w, p);
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

// y = R p_l - o_v (+ t), its part across the ray A y, for observation e
__device__ inline void across_ray(const StartLds& S, int e, const double* R, double tx, double ty, double tz, double* rp, double* az) {
  const int l = S.lm[e], v = S.view[e];
  const double px = S.pl[l][0], py = S.pl[l][1], pz = S.pl[l][2];
  rp[0] = R[0] * px + R[1] * py + R[2] * pz;
  rp[1] = R[3] * px + R[4] * py + R[5] * pz;
  rp[2] = R[6] * px + R[7] * py + R[8] * pz;
  const double z0 = rp[0] + tx - S.org[v][0], z1 = rp[1] + ty - S.org[v][1], z2 = rp[2] + tz - S.org[v][2];
  const double d0 = S.d[e][0], d1 = S.d[e][1], d2 = S.d[e][2];
  const double along = d0 * z0 + d1 * z1 + d2 * z2;
  az[0] = z0 - d0 * along; az[1] = z1 - d1 * along; az[2] = z2 - d2 * along;
}

// t = -(sum w A)^-1 sum w A (R p_l - o_v), `l` the Cholesky factor of sum w A
__device__ inline void solve_translation(const StartLds& S, int n_obs, const Sym3& l, const double* R, double* t) {
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int e = 0; e < n_obs; ++e) {
    double rp[3], az[3];
    across_ray(S, e, R, 0.0, 0.0, 0.0, rp, az);
    const double w = S.wt[e];
    b0 += w * az[0]; b1 += w * az[1]; b2 += w * az[2];
  }
  chol3_solve(l, -b0, -b1, -b2, t);
}

template <int KIND>
__global__ __launch_bounds__(64 * STV_P) void start_pose_views_kernel(const StartViewsArgs a) {
  __shared__ StartLds s_all[STV_P];
  constexpr int ROW = KIND == PROJECT_FISHEYE62 ? 32 : 24;
  const FitViewsArgs& g = a.views;
  const int row = blockIdx.x * STV_P + (threadIdx.x >> 6);
  if (row >= g.pose.n * a.n_bank) return;             // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  const int i = row / a.n_bank, k = row - i * a.n_bank;
  const int32_t* rows = g.cam_rows + (size_t)i * g.max_views;
  // index check: a row outside [-1, n_rows) anywhere in the hand and none of its starts writes anything
  bool bad_row = false;
  for (int v = 0; v < g.max_views; ++v) {
    const int r = rows[v];
    bad_row |= r < -1 || r >= g.n_rows;
  }
  if (bad_row) {
    if (lane == 0) atomicOr(g.status, UT_BAD_SRC_INDEX);
    return;
  }
  StartLds& S = s_all[threadIdx.x >> 6];
  const int mrow = g.pose.n_models == 1 ? 0 : i;
  const bool mirrored = g.pose.mirror && g.pose.mirror[i] == 1;

  // ---- the bank pose's landmarks under the identity wrist
  for (int e = lane; e < 321; e += 64) S.hm[e] = g.pose.hand_model[(size_t)mrow * 321 + e];
  float ang = 0.f;
  if (lane < 20) {
    ang = a.bank[(size_t)k * 20 + lane];
    if (g.pose.limits) ang = fminf(fmaxf(ang, g.pose.limits[(size_t)mrow * 40 + 2 * lane]), g.pose.limits[(size_t)mrow * 40 + 2 * lane + 1]);
    S.ang[lane] = ang;
  }
  if (lane < 12) S.wrist[lane] = lane == 0 ? (mirrored ? -1.f : 1.f) : ((lane == 5 || lane == 10) ? 1.f : 0.f);
  if (lane < 21) { S.w[lane] = 0.f; S.target[lane][0] = 0.f; S.target[lane][1] = 0.f; S.target[lane][2] = 0.f; }
  wave_sync();
  float unused;
  fit_eval(S, S.ang, S.wrist, lane, unused);
  if (lane < 21) { S.pl[lane][0] = S.p[lane][0]; S.pl[lane][1] = S.p[lane][1]; S.pl[lane][2] = S.p[lane][2]; }

  // ---- the used observations, views ascending, by fit_views.hip's rules
  bool bad = false;
  float wl = 0.f;
  int n_obs = 0, first_view = -1;
  unsigned long long seen_landmarks = 0;
  for (int v = 0; v < g.max_views; ++v) {
    const int r = rows[v];
    if (r < 0) continue;
    const double* cam = g.table + (size_t)r * ROW;
    bool used = false;
    float w = 0.f;
    double u[2] = {0.0, 0.0};
    if (lane < 21) {
      const size_t o = ((size_t)i * g.max_views + v) * 21 + lane;
      w = g.weights ? g.weights[o] : 1.f;
      if (!(w >= 0.f && w <= 3.0e38f)) {
        bad = true;
      } else if (w > 0.f) {
        u[0] = g.window[2 * o]; u[1] = g.window[2 * o + 1];
        if (!(finite_d(u[0]) && finite_d(u[1]))) bad = true;
        else { used = true; wl += w; }
      }
    }
    const unsigned long long m = __ballot(used);
    if (used) {
      const int e = n_obs + __popcll(m & ((1ull << lane) - 1ull));
      double d[3];
      start_ray<KIND>(cam, u, d);
      S.d[e][0] = d[0]; S.d[e][1] = d[1]; S.d[e][2] = d[2];
      S.win[e][0] = u[0]; S.win[e][1] = u[1];
      S.wt[e] = (double)w;
      S.view[e] = (unsigned char)v; S.lm[e] = (unsigned char)lane;
    }
    if (lane == 0) {
      const double* t = cam + (KIND == PROJECT_FISHEYE62 ? 21 : 13);
      S.org[v][0] = t[0]; S.org[v][1] = t[1]; S.org[v][2] = t[2];
      S.rows[v] = r;
    }
    if (m && first_view < 0) first_view = v;
    n_obs += __popcll(m);
    seen_landmarks |= m;
  }
  bad = bad || !(wl <= 3.0e38f);
  bool refused = wave_any(bad) || __popcll(seen_landmarks) < 3;
  wave_sync();

  // ---- sum w A and its factor: the same values in every lane
  Sym3 l{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double wsum = 0.0, pc[3] = {0.0, 0.0, 0.0};
  if (!refused) {
    Sym3 m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = 0; e < n_obs; ++e) {
      const double w = S.wt[e], d0 = S.d[e][0], d1 = S.d[e][1], d2 = S.d[e][2];
      const int lm = S.lm[e];
      m.a00 += w * (1.0 - d0 * d0); m.a10 -= w * (d1 * d0); m.a11 += w * (1.0 - d1 * d1);
      m.a20 -= w * (d2 * d0);       m.a21 -= w * (d2 * d1); m.a22 += w * (1.0 - d2 * d2);
      wsum += w;
      pc[0] += w * S.pl[lm][0]; pc[1] += w * S.pl[lm][1]; pc[2] += w * S.pl[lm][2];
    }
    pc[0] /= wsum; pc[1] /= wsum; pc[2] /= wsum;
    refused = !chol3(m, TRI_PIVOT_FRACTION * fmax(m.a00, fmax(m.a11, m.a22)), l);
  }

  // ---- one lane per seed
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  double score = INFINITY, far2 = 0.0;
  if (!refused && lane < a.n_seeds) {
    const double* rc = g.table + (size_t)S.rows[first_view] * ROW + (KIND == PROJECT_FISHEYE62 ? 12 : 4);      // eye -> world
    const double* q = a.seeds + (size_t)lane * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = rc[3 * r] * q[c] + rc[3 * r + 1] * q[3 + c] + rc[3 * r + 2] * q[6 + c];
    for (int it = 0; it < a.iters; ++it) {
      solve_translation(S, n_obs, l, R, t);
      double h[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, rot[3][3];
      for (int e = 0; e < n_obs; ++e) {
        double rp[3], az[3];
        across_ray(S, e, R, t[0], t[1], t[2], rp, az);
        const int lm = S.lm[e];
        const double w = S.wt[e];
        const double p0 = S.pl[lm][0] - pc[0], p1 = S.pl[lm][1] - pc[1], p2 = S.pl[lm][2] - pc[2];
        const double rc0 = R[0] * pc[0] + R[1] * pc[1] + R[2] * pc[2], rc1 = R[3] * pc[0] + R[4] * pc[1] + R[5] * pc[2],
                     rc2 = R[6] * pc[0] + R[7] * pc[1] + R[8] * pc[2];
        const double f0 = (rp[0] - rc0) - az[0], f1 = (rp[1] - rc1) - az[1], f2 = (rp[2] - rc2) - az[2];      // foot point - (R pc + t)
        h[0][0] += w * p0 * f0; h[0][1] += w * p0 * f1; h[0][2] += w * p0 * f2;
        h[1][0] += w * p1 * f0; h[1][1] += w * p1 * f1; h[1][2] += w * p1 * f2;
        h[2][0] += w * p2 * f0; h[2][1] += w * p2 * f1; h[2][2] += w * p2 * f2;
      }
      kabsch_rotation(h, rot);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = rot[r][c];
    }
    solve_translation(S, n_obs, l, R, t);
    // the score: the squared cost of the fit in the views at R p_l + t
    double sum = 0.0;
    bool good = true;
    for (int e = 0; e < n_obs; ++e) {
      const int lm = S.lm[e];
      const double px = S.pl[lm][0], py = S.pl[lm][1], pz = S.pl[lm][2];
      const double X[3] = {R[0] * px + R[1] * py + R[2] * pz + t[0], R[3] * px + R[4] * py + R[5] * pz + t[1],
                           R[6] * px + R[7] * py + R[8] * pz + t[2]};
      double w2[2], ez;
      project_window<KIND>(g.table + (size_t)S.rows[S.view[e]] * ROW, X, w2, ez);
      const double r0 = w2[0] - S.win[e][0], r1 = w2[1] - S.win[e][1];
      const double d2 = r0 * r0 + r1 * r1;
      if (KIND == PROJECT_PINHOLE && !(ez >= TRI_NEAR_Z)) good = false;
      sum += S.wt[e] * d2;
      far2 = fmax(far2, d2);
    }
    if (good && finite_d(sum)) score = sum;
  }

  // ---- the lowest score, the lowest lane among equals
  int best = lane;
  double best_score = score;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(best_score, o);
    const int ol = __shfl_xor(best, o);
    if (os < best_score || (os == best_score && ol < best)) { best_score = os; best = ol; }
  }
  refused = refused || !(best_score < INFINITY);

  float* ja = g.pose.ja + (size_t)row * g.pose.ja_stride;
  float* xf = g.pose.xf + (size_t)row * g.pose.xf_stride;
  if (lane < 22) ja[lane] = lane < 20 ? ang : 0.f;
  if (refused ? lane == 0 : lane == best) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) xf[4 * r + c] = refused ? (r == c ? 1.f : 0.f) : (float)R[3 * r + c];
      xf[4 * r + 3] = refused ? 0.f : (float)t[r] / g.pose.t_scale;
    }
    if (g.pose.xf_stride >= 16) { xf[12] = 0.f; xf[13] = 0.f; xf[14] = 0.f; xf[15] = 1.f; }
    if (g.info) {
      float* o = g.info + (size_t)row * 4;
      o[0] = refused ? 0.f : (float)sqrt(score / wsum);
      o[1] = refused ? 0.f : (float)sqrt(far2);
      o[2] = refused ? -1.f : (float)lane;
      o[3] = refused ? (float)FIT_REFUSED : 0.f;
    }
  }
}

// One wave per hand: every lane walks the candidates' info rows alike, then lanes copy the chosen one.
__global__ __launch_bounds__(256) void select_pose_kernel(const SelectPoseArgs a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int lane = threadIdx.x & 63;
  const float* info = a.info + (size_t)i * a.n_cand * 4;
  int best = -1;
  float best_v = 0.f;
  for (int c = 0; c < a.n_cand; ++c) {
    if ((int)info[4 * c + 3] & FIT_REFUSED) continue;
    const float v = info[4 * c];
    if (best < 0 || v < best_v || (best_v != best_v && v == v)) { best = c; best_v = v; }      // a NaN loses to any number
  }
  const size_t src = (size_t)i * a.n_cand + (best < 0 ? 0 : best);
  if (lane < 22) a.out_ja[(size_t)i * a.out_ja_stride + lane] = a.ja[src * a.ja_stride + lane];
  if (lane < 12) a.out_xf[(size_t)i * a.out_xf_stride + lane] = a.xf[src * a.xf_stride + lane];
  else if (lane < 16 && a.out_xf_stride >= 16) a.out_xf[(size_t)i * a.out_xf_stride + lane] = lane == 15 ? 1.f : 0.f;
  if (a.out_info && lane < 4) a.out_info[(size_t)i * 4 + lane] = a.info[src * 4 + lane];
  if (a.out_index && lane == 0) a.out_index[i] = best;
}

}  // namespace

hipError_t launch_start_pose_views(const StartViewsArgs& a, hipStream_t s) {
  const FitViewsArgs& g = a.views;
  if (g.pose.n <= 0) return hipSuccess;
  if (g.max_views < 1 || g.max_views > TRI_MAX_VIEWS || a.n_bank < 1 || a.n_seeds < 1 || a.n_seeds > 64) return hipErrorInvalidValue;
  const long long total = (long long)g.pose.n * a.n_bank;
  if (total > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + STV_P - 1) / STV_P)), block(64 * STV_P);
  if (g.kind == PROJECT_FISHEYE62) hipLaunchKernelGGL(start_pose_views_kernel<PROJECT_FISHEYE62>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(start_pose_views_kernel<PROJECT_PINHOLE>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_select_pose(const SelectPoseArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(select_pose_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
