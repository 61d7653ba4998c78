// The pose fit of fit.hip with the hand's scale as a 27th parameter, fp32, and the pool that turns per-pose scales into one:
// ut_fit_pose_scale and ut_pool_scale (include/umetrack_hip_scale.h).  The reference calibrates a hand's scale only through
// its network (run_eval_unknown_skeleton.py:55-76); the yardstick is the float64 restatement in tests/scale_cases.py, whose
// constants and decisions this file follows line by line.
//
// Scale s means hand.scaled_hand_model(model, s): the 66 joint and 63 landmark rest coordinates times s in fp32, nothing
// else.  The solver is fit.hip's - same constants, accept / reject rule, Marquardt scaling with its floor, lambda schedule and
// stop rules - on 27 parameters: sigma = ln s is ordered last, d landmark / d sigma = landmark - wrist translation (every
// length grows about the wrist frame's origin), the trial scale is clamp(s exp(d sigma), SCALE_MIN, SCALE_MAX), and a small
// step also needs |d sigma| <= FIT_STEP_TOL.  Every trial writes the pose's LDS model again from an unscaled copy of those
// 129 floats and evaluates ut_fk's arithmetic (ut_fk.h) on it: ut_fk on the blob of scaled_hand_model(model, s) with the
// output pose reproduces the residual the solver saw.  After the loop the scale information of the accepted state: the
// square of the last pivot of the Cholesky factorisation of A + SCALE_INFO_LAMBDA D, i.e. the Schur complement of sigma.
//
// Structure as in fit.hip, with which it shares ut_fit_dev.h (fit.hip compiles to the code it had): one wave per pose,
// FITS_P poses per workgroup, each wave in an LDS region of its own, NO workgroup barrier, no atomics, wave-uniform control
// flow, every private array indexed statically.  A region is 16416 bytes (row stride 29: odd, like fit.hip's 27), so three
// poses share the 64 KB of static LDS a workgroup gets; a fourth would need 65664.
#include <math.h>

#include "ut_fit_dev.h"
#include "ut_fk.h"
#include "ut_kernels.h"
#include "ut_math.h"

namespace ut {
namespace {

constexpr int FITS_P = 3;         // poses (waves) per workgroup
constexpr int FITS_LD = 29;       // row stride of J (27 columns + residual) and of the 28 x 28 normal matrix
constexpr int FITS_NP = 27;       // parameters
constexpr int FITS_SIGMA = 26;    // column of sigma = ln s
constexpr float FIT_LAMBDA_START = 1e-3f, FIT_LAMBDA_DOWN = 0.1f, FIT_LAMBDA_UP = 10.f, FIT_LAMBDA_MIN = 1e-9f;
constexpr float FIT_LAMBDA_CONVERGED_MAX = 1.f;
constexpr float FIT_DIAG_FLOOR = 1e-10f;
constexpr float FIT_STEP_TOL = 1e-5f;
constexpr float FIT_DECREASE_TOL = 1e-3f;
constexpr float FIT_FLAT_TOL = 1e-6f;

struct FitScaleLds {              // one wave's region
  float hm[321];                  // the pose's packed model at the scale of the last evaluated state
  float rest[129];                // its joint (66) and landmark (63) rest coordinates as given: hm[66..194] = rest * scale
  float local[20][12];            // joint transforms of the last evaluated state
  float prefix[20][12];           // W L0 .. L(j-1) in front of joint 4 f + j
  float frame[17][12];            // skinning frames
  float omega[20][3], cw[20][3];  // joint axes and centres in the world (linearisation)
  float jl[63 * FITS_LD];         // J while the normal matrix is formed, then the Cholesky factor L [27][FITS_LD]
  float a[28][FITS_LD];           // lower triangle of [J r]^T [J r]: A = J^T J, row 27 = g = J^T r
  float ang[20], ang_t[20];       // accepted and trial angles
  float wrist[12], wrist_t[12];   // accepted and trial wrist frame
  float p[21][3];                 // landmarks of the last evaluated state
  float target[21][3], w[21];     // targets (0 where the weight is 0) and weights
};
static_assert(sizeof(FitScaleLds) == 16416 && sizeof(FitScaleLds) * FITS_P <= 65536, "a workgroup's static LDS");

// The model of the region at scale s: the bits of scaled_hand_model.  Called by the whole wave; the caller syncs.
__device__ inline void set_scale(FitScaleLds& S, float s, int lane) {
  for (int e = lane; e < 129; e += 64) S.hm[66 + e] = S.rest[e] * s;
}

// fit.hip's fit_linearise with the sigma column (zero when the scale is fixed) in front of the residual column.
__device__ inline void fit_linearise(FitScaleLds& S, int lane, float sign, float cx, float cy, float cz, bool fixed) {
  for (int e = lane; e < 63 * FITS_LD; e += 64) S.jl[e] = 0.f;
  if (lane < 20) joint_axis_in_world(S.prefix[lane], S.hm + 3 * lane, S.hm + 66 + 3 * lane, S.omega[lane], S.cw[lane]);
  wave_sync();
  if (lane < 21 && S.w[lane] > 0.f) {
    const float sw = sqrtf(S.w[lane]);
    float* row = S.jl + 3 * lane * FITS_LD;      // rows 3 l, 3 l + 1, 3 l + 2
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
      const float scale = sw * sign * we;
      for (int j = 0; j <= m; ++j) {
        const int k = 4 * c + j;
        const float vx = yx - S.cw[k][0], vy = yy - S.cw[k][1], vz = yz - S.cw[k][2];
        const float ox = S.omega[k][0], oy = S.omega[k][1], oz = S.omega[k][2];
        row[k] += scale * (oy * vz - oz * vy);
        row[FITS_LD + k] += scale * (oz * vx - ox * vz);
        row[2 * FITS_LD + k] += scale * (ox * vy - oy * vx);
      }
    }
    const float px = S.p[lane][0], py = S.p[lane][1], pz = S.p[lane][2];
    const float vx = px - cx, vy = py - cy, vz = pz - cz;
    // wrist rotation about the centroid: -hat(v); translation: I
    row[21] = sw * vz;            row[22] = -sw * vy;
    row[FITS_LD + 20] = -sw * vz;  row[FITS_LD + 22] = sw * vx;
    row[2 * FITS_LD + 20] = sw * vy; row[2 * FITS_LD + 21] = -sw * vx;
    row[23] = sw; row[FITS_LD + 24] = sw; row[2 * FITS_LD + 25] = sw;
    if (!fixed) {                                 // d landmark / d ln s
      row[FITS_SIGMA] = sw * (px - S.wrist[3]);
      row[FITS_LD + FITS_SIGMA] = sw * (py - S.wrist[7]);
      row[2 * FITS_LD + FITS_SIGMA] = sw * (pz - S.wrist[11]);
    }
    row[27] = sw * (px - S.target[lane][0]);
    row[FITS_LD + 27] = sw * (py - S.target[lane][1]);
    row[2 * FITS_LD + 27] = sw * (pz - S.target[lane][2]);
  }
  wave_sync();
  // 28 * 29 / 2 = 406 entries (i, j <= i), 7 per lane
  for (int e = lane; e < 406; e += 64) {
    int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    if (i * (i + 1) / 2 > e) --i;
    if ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    float s = 0.f;
#pragma unroll 9
    for (int r = 0; r < 63; ++r) s = fmaf(S.jl[r * FITS_LD + i], S.jl[r * FITS_LD + j], s);
    S.a[i][j] = s;
  }
  wave_sync();
}

// The factorisation alone, for the scale information: the last pivot of A + lambda D, 0 when a pivot is not positive and
// finite.  No LDS traffic beyond reading S.a.
__device__ inline float fit_last_pivot(FitScaleLds& S, int lane, float lambda, float diag) {
  const bool row = lane < FITS_NP;
  float a[FITS_NP];
#pragma unroll
  for (int k = 0; k < FITS_NP; ++k) a[k] = (row && k <= lane) ? S.a[row ? lane : 0][k] + (k == lane ? lambda * diag : 0.f) : 0.f;
  float piv = 0.f;
#pragma unroll
  for (int j = 0; j < FITS_NP; ++j) {
    piv = lane_value(a[j], j);
    if (!(piv > 0.f) || !(piv <= 3.0e38f)) return 0.f;
    a[j] *= 1.f / sqrtf(piv);
#pragma unroll
    for (int k = j + 1; k < FITS_NP; ++k) a[k] = fmaf(-a[j], lane_value(a[j], k), a[k]);
  }
  return piv;
}

__global__ __launch_bounds__(64 * FITS_P) void fit_pose_scale_kernel(const FitScaleArgs a) {
  __shared__ FitScaleLds s_all[FITS_P];
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * FITS_P + (threadIdx.x >> 6);
  if (i >= a.n) return;                               // whole waves leave; nobody waits for them
  FitScaleLds& S = s_all[threadIdx.x >> 6];
  const int mrow = a.n_models == 1 ? 0 : i;
  const bool warm = a.init_ja != nullptr;
  const bool mirrored = a.mirror && a.mirror[i] == 1;
  const bool fixed = a.scale_mode == FITS_MODE_FIXED;
  const float sign = mirrored ? -1.f : 1.f;

  // ---- inputs: the model and its unscaled rest coordinates, the start's scale, the targets of weighted landmarks (others
  // are never read), the box, the start
  for (int e = lane; e < 321; e += 64) S.hm[e] = a.hand_model[(size_t)mrow * 321 + e];
  for (int e = lane; e < 129; e += 64) S.rest[e] = a.hand_model[(size_t)mrow * 321 + 66 + e];
  float scale = a.init_scale ? a.init_scale[i] : 1.f;
  const bool bad_scale = !(scale >= FITS_SCALE_MIN) || !(scale <= FITS_SCALE_MAX);      // a NaN is neither
  if (bad_scale) scale = 1.f;
  float wl = 0.f;
  bool bad = false;
  if (lane < 21) {
    wl = a.weights ? a.weights[(size_t)i * 21 + lane] : 1.f;
    bad = !(wl >= 0.f) || !(wl <= 3.0e38f);
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (!bad && wl > 0.f) {
      const float* t = a.targets + (size_t)i * a.target_stride + 3 * lane;
      tx = t[0]; ty = t[1]; tz = t[2];
      bad = !(fabsf(tx) <= 3.0e38f) || !(fabsf(ty) <= 3.0e38f) || !(fabsf(tz) <= 3.0e38f);
    }
    if (bad) wl = 0.f;
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
  bool refused = wave_any(bad) || __popcll(__ballot(wl > 0.f)) < 3 || bad_scale;
  const float wsum = wave_sum(wl);
  float cx = 0.f, cy = 0.f, cz = 0.f, extent = 0.f;
  wave_sync();
  set_scale(S, scale, lane);                          // after the sync: S.rest is written by other lanes
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
    // ---- cold start: the rest pose (inside the box) of the model at the start's scale, aligned to the targets by a weighted
    // Kabsch fit of its landmarks.  H and the rotation in fp64 (ut_math.h), every lane the same values.
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
    cost = fit_eval(S, S.ang, S.wrist, lane, worst);
    if (!(cost <= 3.0e38f)) { refused = true; keep_start = false; }      // a start that is not finite
  }

  int iters = 0, status = refused ? FITS_REFUSED : 0;
  float scale_info = 0.f;
  if (!refused) {
    float lambda = FIT_LAMBDA_START, diag = 0.f;
    bool fresh = true, done = false;
    for (; iters < a.max_iters && !done;) {
      if (fresh) {
        fit_linearise(S, lane, sign, cx, cy, cz, fixed);
        const float d = lane < FITS_NP ? S.a[lane][lane] : 0.f;
        diag = fmaxf(d, FIT_DIAG_FLOOR * wave_max(d));
        fresh = false;
      }
      float delta = 0.f;
      const bool ok = fit_solve<FITS_NP, FITS_LD>(S, lane, lambda, diag, delta);
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
      // with the sigma column zero the floored diagonal gives d sigma = 0; the fixed scale is kept by construction as well
      const float ds = fixed ? 0.f : lane_value(delta, FITS_SIGMA);
      const float scale_t = fixed ? scale : fminf(fmaxf(scale * expf(ds), FITS_SCALE_MIN), FITS_SCALE_MAX);
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
      set_scale(S, scale_t, lane);
      const bool step_small = wave_max(step) <= FIT_STEP_TOL &&
                              fmaxf(fabsf(rx), fmaxf(fabsf(ry), fabsf(rz))) <= FIT_STEP_TOL &&
                              fmaxf(fabsf(ux), fmaxf(fabsf(uy), fabsf(uz))) <= FIT_STEP_TOL * extent &&
                              fabsf(ds) <= FIT_STEP_TOL;
      wave_sync();
      float worst_t;
      const float cost_t = fit_eval(S, S.ang_t, S.wrist_t, lane, worst_t);
      const bool accept = cost_t < cost;              // false for a NaN; +inf cannot be below a finite cost
      const bool flat = !accept || cost - cost_t <= FIT_DECREASE_TOL * cost;
      const bool stationary = !accept && fabsf(cost_t - cost) <= FIT_FLAT_TOL * cost;      // false for a NaN
      done = (step_small && flat && lambda <= FIT_LAMBDA_CONVERGED_MAX) || stationary;
      if (accept) {
        if (lane < 20) S.ang[lane] = S.ang_t[lane];
        if (lane < 12) S.wrist[lane] = S.wrist_t[lane];
        cost = cost_t; worst = worst_t; scale = scale_t;
        lambda = fmaxf(lambda * FIT_LAMBDA_DOWN, FIT_LAMBDA_MIN);
        fresh = true;
        wave_sync();
      } else {
        lambda *= FIT_LAMBDA_UP;
      }
    }
    status = done ? FITS_CONVERGED : FITS_AT_MAX_ITERS;
    if (!fixed) {
      // ---- the scale information at the accepted state.  After an accepted last trial LDS holds that state (model at its
      // scale, frames, landmarks) and the normal matrix is the one before it: linearise once more.  After a rejected one the
      // normal matrix is the accepted state's already, and nothing else is needed.
      if (fresh) fit_linearise(S, lane, sign, cx, cy, cz, false);
      const float d = lane < FITS_NP ? S.a[lane][lane] : 0.f;
      diag = fmaxf(d, FIT_DIAG_FLOOR * wave_max(d));
      scale_info = uniform(fit_last_pivot(S, lane, FITS_SCALE_INFO_LAMBDA, diag));
      if (scale <= FITS_SCALE_MIN || scale >= FITS_SCALE_MAX) status |= FITS_AT_BOUND;
    }
  }

  // ---- outputs: a refused pose gives back its start - the rest pose at the identity on a cold start, and when the start
  // itself is what was refused (its cost is not finite) - and scale 1
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
  if (lane == 0) a.scale[i] = refused ? 1.f : scale;
  if (a.info && lane == 0) {
    float* o = a.info + (size_t)i * 6;
    o[0] = refused ? 0.f : sqrtf(cost / wsum);
    o[1] = refused ? 0.f : worst;
    o[2] = (float)iters;
    o[3] = (float)status;
    o[4] = scale_info;
    o[5] = 0.f;
  }
}

// One wave per group of group_size consecutive poses: the information-weighted mean of ln s in fp64.  Lanes stride over the
// group in a fixed order and the sums go through the butterfly, so a group's row depends on its own poses alone.
__global__ __launch_bounds__(64) void pool_scale_kernel(const float* __restrict__ scale, const float* __restrict__ info,
                                                        int group_size, float* __restrict__ group,
                                                        float* __restrict__ pose_scale) {
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * group_size;
  double si = 0.0, sil = 0.0, cnt = 0.0;
  for (int k = lane; k < group_size; k += 64) {
    const float* o = info + (base + k) * 6;
    const int status = (int)o[3];
    const float inf = o[4];
    const bool use = (status & FITS_CONVERGED) && !(status & (FITS_REFUSED | FITS_AT_BOUND)) && inf > 0.f && inf <= 3.0e38f;
    if (use) {
      const double l = log((double)scale[base + k]);
      si += (double)inf; sil += (double)inf * l; cnt += 1.0;
    }
  }
  si = wave_sum(si); sil = wave_sum(sil); cnt = wave_sum(cnt);
  const bool any = cnt > 0.0;
  const double mean = any ? sil / si : 0.0;
  double ss = 0.0;
  for (int k = lane; k < group_size; k += 64) {
    const float* o = info + (base + k) * 6;
    const int status = (int)o[3];
    const float inf = o[4];
    const bool use = (status & FITS_CONVERGED) && !(status & (FITS_REFUSED | FITS_AT_BOUND)) && inf > 0.f && inf <= 3.0e38f;
    if (use) {
      const double dl = log((double)scale[base + k]) - mean;
      ss += (double)inf * dl * dl;
    }
  }
  ss = wave_sum(ss);
  const float pooled = any ? (float)exp(mean) : 1.f;
  if (lane == 0) {
    float* g = group + (size_t)blockIdx.x * 4;
    g[0] = pooled;
    g[1] = any ? (float)(1.0 / sqrt(si)) : __int_as_float(0x7f800000);
    g[2] = any ? (float)sqrt(ss / fmax(cnt - 1.0, 1.0)) : 0.f;
    g[3] = (float)cnt;
  }
  if (pose_scale)
    for (int k = lane; k < group_size; k += 64) pose_scale[base + k] = pooled;
}

}  // namespace

hipError_t launch_fit_pose_scale(const FitScaleArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fit_pose_scale_kernel, dim3((a.n + FITS_P - 1) / FITS_P), dim3(64 * FITS_P), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_scale(const float* scale, const float* info, int n_groups, int group_size, float* group,
                             float* pose_scale, hipStream_t s) {
  if (n_groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(pool_scale_kernel, dim3(n_groups), dim3(64), 0, s, scale, info, group_size, group, pose_scale);
  return hipGetLastError();
}

}  // namespace ut
