// The pose fit of fit.hip on landmarks that come with their information, fp32: ut_fit_pose_info (include/umetrack_hip_info.h).
// Every landmark l brings the lower Cholesky factor L_l of a 3 x 3 information matrix H_l = L_l L_l^T - six floats, what
// ut_triangulate_points_info hands out - and the cost is sum_l |L_l^T (landmark_l - target_l)|^2: one Gauss-Newton
// linearisation of the reprojection cost about the triangulated points.  The yardstick is the float64 restatement in
// tests/info_cases.py, whose decisions this file follows line by line.
//
// The solver is fit.hip's - same 26 parameters, constants, accept / reject rule, Marquardt scaling with its floor, lambda
// schedule and stop rules, the solve of ut_fit_dev.h - on 63 whitened rows: the three Jacobian rows (and the residual
// column) of a landmark are filled as fit.hip fills them, without the sqrt(weight), and the landmark's lane then replaces
// the 27 columns a = (a0, a1, a2) of its rows by L^T a in place: (l00 a0 + l10 a1 + l20 a2, l11 a1 + l21 a2, l22 a2).  The
// forward function is fit_eval's (ut_fk's arithmetic); its isotropic cost is dropped and the whitened one summed behind it.
// A landmark is used when any entry of its factor is non-zero; its scalar weight - for the centroid the wrist turns about,
// the extent and the cold start's Kabsch fit - is |L|_F^2 = trace(H).
//
// Structure as in fit.hip (which compiles to the code it had): one wave per pose, FITI_P poses per workgroup, each wave in an
// LDS region of its own, NO workgroup barrier, no atomics, wave-uniform control flow, every private array indexed
// statically.  The factors add 504 bytes to a region: 4 x 15568 = 62272 bytes of the 64 KB a workgroup gets.
#include <math.h>

#include "ut_fit_dev.h"
#include "ut_fk.h"
#include "ut_kernels.h"
#include "ut_math.h"

namespace ut {
namespace {

constexpr int FITI_P = 4;        // poses (waves) per workgroup
constexpr int FITI_LD = 27;      // row stride of J (26 columns + residual) and of the 27 x 27 normal matrix: odd, like fit.hip's
constexpr int FITI_NP = 26;      // parameters
constexpr float FIT_LAMBDA_START = 1e-3f, FIT_LAMBDA_DOWN = 0.1f, FIT_LAMBDA_UP = 10.f, FIT_LAMBDA_MIN = 1e-9f;
constexpr float FIT_LAMBDA_CONVERGED_MAX = 1.f;
constexpr float FIT_DIAG_FLOOR = 1e-10f;
constexpr float FIT_STEP_TOL = 1e-5f;
constexpr float FIT_DECREASE_TOL = 1e-3f;
constexpr float FIT_FLAT_TOL = 1e-6f;
enum : int { FIT_CONVERGED = 1, FIT_AT_MAX_ITERS = 2, FIT_REFUSED = 4 };      // UT_FIT_*

struct FitInfoLds {              // one wave's region, 15568 bytes: FITI_P of them stay inside the 64 KB a workgroup gets
  float hm[321];                 // the pose's packed model
  float local[20][12];           // joint transforms of the last evaluated state
  float prefix[20][12];          // W L0 .. L(j-1) in front of joint 4 f + j
  float frame[17][12];           // skinning frames
  float omega[20][3], cw[20][3]; // joint axes and centres in the world (linearisation)
  float jl[63 * FITI_LD];        // J while the normal matrix is formed, then the Cholesky factor L [26][FITI_LD]
  float a[27][FITI_LD];          // lower triangle of [J r]^T [J r]: A = J^T J, row 26 = g = J^T r
  float ang[20], ang_t[20];      // accepted and trial angles
  float wrist[12], wrist_t[12];  // accepted and trial wrist frame (translation in target units, column 0 negated if mirrored)
  float p[21][3];                // landmarks of the last evaluated state
  float target[21][3], w[21];    // targets (0 where the landmark is unused) and scalar weights trace(H), 0 = unused
  float li[21][6];               // l00 l10 l11 l20 l21 l22 of every landmark's factor
};
static_assert(sizeof(FitInfoLds) == 15568 && sizeof(FitInfoLds) * FITI_P <= 65536, "a workgroup's static LDS");

// The whitened cost sum_l |L_l^T (p_l - target_l)|^2 of the state fit_eval left in S.p.  Called by the whole wave.
__device__ inline float whitened_cost(const FitInfoLds& S, int lane, bool used) {
  float c = 0.f;
  if (used) {
    const float* l = S.li[lane];
    const float r0 = S.p[lane][0] - S.target[lane][0], r1 = S.p[lane][1] - S.target[lane][1], r2 = S.p[lane][2] - S.target[lane][2];
    const float u0 = l[0] * r0 + l[1] * r1 + l[3] * r2, u1 = l[2] * r1 + l[4] * r2, u2 = l[5] * r2;
    c = u0 * u0 + u1 * u1 + u2 * u2;
  }
  return wave_sum(c);               // carries a NaN of the state
}

// The forward function of (ang, wrist) and its whitened cost; worst: the largest Euclidean residual of a used landmark.
__device__ inline float fit_eval_info(FitInfoLds& S, const float* ang, const float* wrist, int lane, bool used, float& worst) {
  fit_eval(S, ang, wrist, lane, worst);
  return whitened_cost(S, lane, used);
}

// (1): fit.hip's fit_linearise without the sqrt(weight), the three rows of a landmark then whitened in place by its lane, into
// S.jl (residual in column 26); then the lower triangle of [J r]^T [J r] into S.a.  Needs S.prefix / frame / p of the accepted
// state.  sign: determinant of the wrist's linear part.
__device__ inline void fit_linearise(FitInfoLds& S, int lane, bool used, float sign, float cx, float cy, float cz) {
  for (int e = lane; e < 63 * FITI_LD; e += 64) S.jl[e] = 0.f;
  if (lane < 20) joint_axis_in_world(S.prefix[lane], S.hm + 3 * lane, S.hm + 66 + 3 * lane, S.omega[lane], S.cw[lane]);
  wave_sync();
  if (used) {
    float* row = S.jl + 3 * lane * FITI_LD;      // rows 3 l, 3 l + 1, 3 l + 2
    const float* lm = S.hm + 132 + 3 * lane;
    const float* wts = S.hm + 195 + 3 * lane;
    const float* idx = S.hm + 258 + 3 * lane;
    for (int e = 0; e < 3; ++e) {
      const float we = wts[e];
      const int f = (int)idx[e];
      // the dense weight of frame f is the LAST non-zero entry naming it (blend_landmark): earlier ones are dead
      bool live = we != 0.f && f >= 2 && f < 17;
      for (int e2 = e + 1; e2 < 3; ++e2) live = live && !(wts[e2] != 0.f && (int)idx[e2] == f);
      if (!live) continue;
      const int c = (f - 2) / 3, m = (f - 2) - 3 * c + 1;     // the frame after joints 0 .. m of finger c
      const float* t = S.frame[f];
      const float yx = t[0] * lm[0] + t[1] * lm[1] + t[2] * lm[2] + t[3];
      const float yy = t[4] * lm[0] + t[5] * lm[1] + t[6] * lm[2] + t[7];
      const float yz = t[8] * lm[0] + t[9] * lm[1] + t[10] * lm[2] + t[11];
      const float scale = sign * we;
      for (int j = 0; j <= m; ++j) {
        const int k = 4 * c + j;
        const float vx = yx - S.cw[k][0], vy = yy - S.cw[k][1], vz = yz - S.cw[k][2];
        const float ox = S.omega[k][0], oy = S.omega[k][1], oz = S.omega[k][2];
        row[k] += scale * (oy * vz - oz * vy);
        row[FITI_LD + k] += scale * (oz * vx - ox * vz);
        row[2 * FITI_LD + k] += scale * (ox * vy - oy * vx);
      }
    }
    const float px = S.p[lane][0], py = S.p[lane][1], pz = S.p[lane][2];
    const float vx = px - cx, vy = py - cy, vz = pz - cz;
    // wrist rotation about the centroid: -hat(v); translation: I
    row[21] = vz;             row[22] = -vy;
    row[FITI_LD + 20] = -vz;  row[FITI_LD + 22] = vx;
    row[2 * FITI_LD + 20] = vy; row[2 * FITI_LD + 21] = -vx;
    row[23] = 1.f; row[FITI_LD + 24] = 1.f; row[2 * FITI_LD + 25] = 1.f;
    row[26] = px - S.target[lane][0];
    row[FITI_LD + 26] = py - S.target[lane][1];
    row[2 * FITI_LD + 26] = pz - S.target[lane][2];
    // rows <- L^T rows: this lane wrote them, nobody else reads them before the wave_sync below
    const float l00 = S.li[lane][0], l10 = S.li[lane][1], l11 = S.li[lane][2], l20 = S.li[lane][3], l21 = S.li[lane][4],
                l22 = S.li[lane][5];
    for (int c = 0; c < FITI_LD; ++c) {
      const float a0 = row[c], a1 = row[FITI_LD + c], a2 = row[2 * FITI_LD + c];
      row[c] = l00 * a0 + l10 * a1 + l20 * a2;
      row[FITI_LD + c] = l11 * a1 + l21 * a2;
      row[2 * FITI_LD + c] = l22 * a2;
    }
  }
  wave_sync();
  // 27 * 28 / 2 = 378 entries (i, j <= i), 6 per lane
  for (int e = lane; e < 378; e += 64) {
    int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    if (i * (i + 1) / 2 > e) --i;
    if ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    float s = 0.f;
#pragma unroll 9
    for (int r = 0; r < 63; ++r) s = fmaf(S.jl[r * FITI_LD + i], S.jl[r * FITI_LD + j], s);
    S.a[i][j] = s;
  }
  wave_sync();
}

__global__ __launch_bounds__(64 * FITI_P) void fit_pose_info_kernel(const FitInfoArgs a) {
  __shared__ FitInfoLds s_all[FITI_P];
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * FITI_P + (threadIdx.x >> 6);
  if (i >= a.n) return;                               // whole waves leave; nobody waits for them
  FitInfoLds& S = s_all[threadIdx.x >> 6];
  const int mrow = a.n_models == 1 ? 0 : i;
  const bool warm = a.init_ja != nullptr;
  const bool mirrored = a.mirror && a.mirror[i] == 1;
  const float sign = mirrored ? -1.f : 1.f;

  // ---- inputs: the model, the factors, the targets of used landmarks (others are never read), the box, the start
  for (int e = lane; e < 321; e += 64) S.hm[e] = a.hand_model[(size_t)mrow * 321 + e];
  float wl = 0.f;                                     // trace(H) = |L|_F^2, the landmark's scalar weight
  bool bad = false, used = false;
  if (lane < 21) {
    const float* f = a.sqrt_info + ((size_t)i * 21 + lane) * 6;
    float l[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      l[k] = f[k];
      bad = bad || !(fabsf(l[k]) <= 3.0e38f);
      used = used || l[k] != 0.f;
      wl = fmaf(l[k], l[k], wl);
    }
    bad = bad || !(wl <= 3.0e38f);
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (!bad && used) {
      const float* t = a.targets + (size_t)i * a.target_stride + 3 * lane;
      tx = t[0]; ty = t[1]; tz = t[2];
      bad = !(fabsf(tx) <= 3.0e38f) || !(fabsf(ty) <= 3.0e38f) || !(fabsf(tz) <= 3.0e38f);
    }
    if (bad || !used) { wl = 0.f; used = false; }
#pragma unroll
    for (int k = 0; k < 6; ++k) S.li[lane][k] = used ? l[k] : 0.f;
    S.w[lane] = wl;
    S.target[lane][0] = tx; S.target[lane][1] = ty; S.target[lane][2] = tz;
  }
  const bool boxed = a.limits != nullptr;
  float lo = 0.f, hi = 0.f, ang0 = 0.f;
  if (lane < 20) {
    if (boxed) { lo = a.limits[(size_t)mrow * 40 + 2 * lane]; hi = a.limits[(size_t)mrow * 40 + 2 * lane + 1]; }
    if (warm) ang0 = a.init_ja[(size_t)i * a.init_ja_stride + lane];
    if (boxed) ang0 = fminf(fmaxf(ang0, lo), hi);
    S.ang[lane] = ang0;
  }
  float tail = 0.f;                                   // angles 20, 21 do not enter the skinning: copied through
  if (warm && (lane == 20 || lane == 21)) tail = a.init_ja[(size_t)i * a.init_ja_stride + lane];
  float init_w = 0.f;                                 // lanes 0..11: the start's wrist rows as given
  if (lane < 12) {
    init_w = warm ? a.init_xf[(size_t)i * a.init_xf_stride + lane] : ((lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f);
    float v = init_w;
    if ((lane & 3) == 3) v *= a.t_scale;
    if ((lane & 3) == 0 && mirrored) v = -v;
    S.wrist[lane] = v;
  }
  const int n_used = __popcll(__ballot(used));
  bool refused = wave_any(bad) || n_used < 3;
  const float wsum = wave_sum(wl);
  float cx = 0.f, cy = 0.f, cz = 0.f, extent = 0.f;
  wave_sync();
  if (!refused) {
    const float tx = lane < 21 ? S.target[lane][0] : 0.f, ty = lane < 21 ? S.target[lane][1] : 0.f,
                tz = lane < 21 ? S.target[lane][2] : 0.f;
    cx = wave_sum(wl * tx) / wsum; cy = wave_sum(wl * ty) / wsum; cz = wave_sum(wl * tz) / wsum;
    extent = sqrtf(wave_sum(wl * ((tx - cx) * (tx - cx) + (ty - cy) * (ty - cy) + (tz - cz) * (tz - cz))) / wsum);
  }

  float cost = 0.f, worst = 0.f;
  bool keep_start = warm;                             // what a refused pose gives back
  if (!refused && !warm) {
    // ---- cold start: the rest pose (inside the box), aligned to the targets by a weighted Kabsch fit of its landmarks.
    // H and the rotation in fp64 (ut_math.h), every lane the same values.
    float unused;
    fit_eval(S, S.ang, S.wrist, lane, unused);
    const double w = wl, inv = 1.0 / (double)wsum;
    const double qx = lane < 21 ? S.p[lane][0] : 0.0, qy = lane < 21 ? S.p[lane][1] : 0.0, qz = lane < 21 ? S.p[lane][2] : 0.0;
    const double mx = wave_sum(w * qx) * inv, my = wave_sum(w * qy) * inv, mz = wave_sum(w * qz) * inv;
    const double dx = lane < 21 ? S.target[lane][0] - (double)cx : 0.0, dy = lane < 21 ? S.target[lane][1] - (double)cy : 0.0,
                 dz = lane < 21 ? S.target[lane][2] - (double)cz : 0.0;
    double h[3][3], r[3][3];
    h[0][0] = wave_sum(w * (qx - mx) * dx); h[0][1] = wave_sum(w * (qx - mx) * dy); h[0][2] = wave_sum(w * (qx - mx) * dz);
    h[1][0] = wave_sum(w * (qy - my) * dx); h[1][1] = wave_sum(w * (qy - my) * dy); h[1][2] = wave_sum(w * (qy - my) * dz);
    h[2][0] = wave_sum(w * (qz - mz) * dx); h[2][1] = wave_sum(w * (qz - mz) * dy); h[2][2] = wave_sum(w * (qz - mz) * dz);
    kabsch_rotation(h, r);                            // target ~ r (q - mean) + centroid
    wave_sync();
    if (lane == 0) {
      // q already carries the mirror: the frame is r diag(sign, 1, 1), and its translation takes the rest landmarks' mean there
      const double t[3] = {cx - (r[0][0] * mx + r[0][1] * my + r[0][2] * mz), cy - (r[1][0] * mx + r[1][1] * my + r[1][2] * mz),
                           cz - (r[2][0] * mx + r[2][1] * my + r[2][2] * mz)};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        S.wrist[4 * k] = (float)r[k][0] * sign; S.wrist[4 * k + 1] = (float)r[k][1]; S.wrist[4 * k + 2] = (float)r[k][2];
        S.wrist[4 * k + 3] = (float)t[k];
      }
    }
    wave_sync();
  }
  if (!refused) {
    cost = fit_eval_info(S, S.ang, S.wrist, lane, used, worst);
    if (!(cost <= 3.0e38f)) { refused = true; keep_start = false; }      // a start that is not finite
  }

  int iters = 0, status = refused ? FIT_REFUSED : 0;
  if (!refused) {
    float lambda = FIT_LAMBDA_START, diag = 0.f;
    bool fresh = true, done = false;
    for (; iters < a.max_iters && !done;) {
      if (fresh) {
        fit_linearise(S, lane, used, sign, cx, cy, cz);
        const float d = lane < FITI_NP ? S.a[lane][lane] : 0.f;
        diag = fmaxf(d, FIT_DIAG_FLOOR * wave_max(d));
        fresh = false;
      }
      float delta = 0.f;
      const bool ok = fit_solve<FITI_NP, FITI_LD>(S, lane, lambda, diag, delta);
      ++iters;
      if (!ok) { lambda *= FIT_LAMBDA_UP; continue; }
      // ---- trial state
      float step = 0.f;
      if (lane < 20) {
        float t = S.ang[lane] + delta;
        if (boxed) t = fminf(fmaxf(t, lo), hi);
        S.ang_t[lane] = t;
        step = fabsf(t - S.ang[lane]);
      }
      const float rx = lane_value(delta, 20), ry = lane_value(delta, 21), rz = lane_value(delta, 22);
      const float ux = lane_value(delta, 23), uy = lane_value(delta, 24), uz = lane_value(delta, 25);
      float e[9];
      rodrigues(rx, ry, rz, e);
      if (lane < 3) {                                 // row `lane` of [E R | E (t - c) + c + dt]
        const float e0 = lane == 0 ? e[0] : (lane == 1 ? e[3] : e[6]), e1 = lane == 0 ? e[1] : (lane == 1 ? e[4] : e[7]),
                    e2 = lane == 0 ? e[2] : (lane == 1 ? e[5] : e[8]);
        const float* m = S.wrist;
        S.wrist_t[4 * lane] = e0 * m[0] + e1 * m[4] + e2 * m[8];
        S.wrist_t[4 * lane + 1] = e0 * m[1] + e1 * m[5] + e2 * m[9];
        S.wrist_t[4 * lane + 2] = e0 * m[2] + e1 * m[6] + e2 * m[10];
        const float cl = lane == 0 ? cx : (lane == 1 ? cy : cz), ul = lane == 0 ? ux : (lane == 1 ? uy : uz);
        S.wrist_t[4 * lane + 3] = e0 * (m[3] - cx) + e1 * (m[7] - cy) + e2 * (m[11] - cz) + cl + ul;
      }
      const bool step_small = wave_max(step) <= FIT_STEP_TOL &&
                              fmaxf(fabsf(rx), fmaxf(fabsf(ry), fabsf(rz))) <= FIT_STEP_TOL &&
                              fmaxf(fabsf(ux), fmaxf(fabsf(uy), fabsf(uz))) <= FIT_STEP_TOL * extent;
      wave_sync();
      float worst_t;
      const float cost_t = fit_eval_info(S, S.ang_t, S.wrist_t, lane, used, worst_t);
      const bool accept = cost_t < cost;              // false for a NaN; +inf cannot be below a finite cost
      const bool flat = !accept || cost - cost_t <= FIT_DECREASE_TOL * cost;
      const bool stationary = !accept && fabsf(cost_t - cost) <= FIT_FLAT_TOL * cost;      // false for a NaN
      done = (step_small && flat && lambda <= FIT_LAMBDA_CONVERGED_MAX) || stationary;
      if (accept) {
        if (lane < 20) S.ang[lane] = S.ang_t[lane];
        if (lane < 12) S.wrist[lane] = S.wrist_t[lane];
        cost = cost_t; worst = worst_t;
        lambda = fmaxf(lambda * FIT_LAMBDA_DOWN, FIT_LAMBDA_MIN);
        fresh = true;
        wave_sync();
      } else {
        lambda *= FIT_LAMBDA_UP;
      }
    }
    status = done ? FIT_CONVERGED : FIT_AT_MAX_ITERS;
  }

  // ---- outputs: a refused pose gives back its start - the rest pose at the identity on a cold start, and when the start
  // itself is what was refused (its cost is not finite)
  if (lane < 22) {
    float v = refused && !keep_start ? 0.f : tail;
    if (lane < 20) {
      v = refused ? (keep_start ? a.init_ja[(size_t)i * a.init_ja_stride + lane] : 0.f) : S.ang[lane];
      if (!refused && !boxed && fabsf(v) > 3.14159265358979f)
        v -= 6.28318530717959f * ceilf((v - 3.14159265358979f) / 6.28318530717959f);      // into (-pi, pi]
    }
    a.ja[(size_t)i * a.ja_stride + lane] = v;
  }
  if (lane < 12) {
    float v = keep_start ? init_w : ((lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f);
    if (!refused) {
      v = S.wrist[lane];
      if ((lane & 3) == 3) v /= a.t_scale;
      if ((lane & 3) == 0 && mirrored) v = -v;
    }
    a.xf[(size_t)i * a.xf_stride + lane] = v;
  } else if (lane < 16 && a.xf_stride >= 16) {
    a.xf[(size_t)i * a.xf_stride + lane] = lane == 15 ? 1.f : 0.f;
  }
  if (a.info && lane == 0) {
    float* o = a.info + (size_t)i * 4;
    o[0] = refused ? 0.f : sqrtf(cost / (float)(3 * n_used));
    o[1] = refused ? 0.f : worst;
    o[2] = (float)iters;
    o[3] = (float)status;
  }
}

}  // namespace

hipError_t launch_fit_pose_info(const FitInfoArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fit_pose_info_kernel, dim3((a.n + FITI_P - 1) / FITI_P), dim3(64 * FITI_P), 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
