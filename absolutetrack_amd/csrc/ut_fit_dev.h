// The pose fits' solver, written once: fit.hip, fit_scale.hip, fit_info.hip and fit_views.hip each describe a cost and instantiate it.
// At the end the hand's scale as a 27th parameter, FitScaleParam, which fit_scale.hip and fit_views_scale.hip share.
//
// Levenberg-Marquardt on NP parameters (20 angle increments, a wrist rotation about the weighted centroid of the targets, a
// wrist translation, then whatever the problem adds) and 63 residual rows, Marquardt's diagonal scaling with a floor, Cholesky
// solve, a trial accepted only when the cost goes down.  The yardsticks are the float64 restatements in tests/fit_cases.py,
// scale_cases.py and info_cases.py, whose constants and decisions fit_pose() below follows line by line.
//
// One wave per pose, every wave in an LDS region of its own: trip counts differ per pose, so there is NO workgroup barrier
// anywhere - waves order their own LDS traffic with wave_sync() - no atomics, and a pose's bits cannot depend on its
// neighbours.  Every loop bound and branch on solver state is wave uniform (reductions are butterflies, which leave the same
// bits in every lane, and go through uniform()), and every private array is indexed statically.  Everything here is
// __device__ inline, so that the LDS address space of a region is inferred in the one kernel that inlines it.
//
// Phases of one iteration (lanes of the pose's wave):
//  (1) linearise, only after an accepted step: joint axes in the world from the prefix frames (20 lanes), three Jacobian rows
//      per landmark with the residual as column NP (one lane per landmark, sparse: a landmark moves with the joints of the
//      frames that carry it), J^T J and J^T r as one lower triangle of (NP + 1)^2 dot products
//  (2) factor A + lambda D right-looking with one lane per row and the row in registers (fully unrolled, cross-lane values by
//      v_readlane on constant lanes, no LDS); forward solve the same way, backward solve on the factor transposed through LDS
//  (3) trial state (angles clamped to the optional box, wrist <- exp(dr) about the centroid, + dt) and its forward
//      function: joint transforms (20 lanes), finger chains (5 lanes), landmark blend and residual (21 lanes) - the code
//      of fk.hip (ut_fk.h), so the residual is ut_fk's arithmetic
//  (4) accept / reject, lambda, convergence.
//
// A problem `P` is a small per-lane object with
//   P::Lds, P::NP, P::LD   the LDS region (the members fit.hip's FitLds documents, plus the problem's own), the parameter
//                          count, and the row stride of J and of the normal matrix: odd, so that lanes reading one column
//                          of consecutive rows hit distinct banks
//   load        a landmark's scalar weight and whether it is used and valid, and whatever else the problem reads
//   row_scale   the factor on a landmark's three Jacobian rows (sqrt(weight), or 1 when finish_rows weighs them)
//   finish_rows what a landmark's lane adds to its rows behind the common columns
//   cost        the cost of the state fit_eval just evaluated
//   trial       what else a trial changes; whether that change is small
//   keep        the trial's extra state becomes the accepted one
//   report      what is written besides the pose and the wrist
// A problem without 3-D targets (fit_views.hip) declares `static constexpr bool PIVOT_FROM_START = true`: nothing is read
// through FitPoseArgs::targets, S.target stays 0, and the pivot of the wrist increment and the extent behind the translation's
// step tolerance are the weighted centroid and extent of the START's landmarks.  Compile time only: the other problems
// compile to what they compiled to without it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "ut_fk.h"
#include "ut_kernels.h"
#include "ut_math.h"

namespace ut {

constexpr float FIT_LAMBDA_START = 1e-3f, FIT_LAMBDA_DOWN = 0.1f, FIT_LAMBDA_UP = 10.f, FIT_LAMBDA_MIN = 1e-9f;
constexpr float FIT_LAMBDA_CONVERGED_MAX = 1.f;   // a small step under heavy damping is a stall, not convergence
constexpr float FIT_DIAG_FLOOR = 1e-10f;          // relative to the largest diagonal entry of J^T W J
constexpr float FIT_STEP_TOL = 1e-5f;             // rad (angles, wrist rotation); x the targets' extent (translation)
constexpr float FIT_DECREASE_TOL = 1e-3f;         // relative cost decrease of an accepted step
constexpr float FIT_FLAT_TOL = 1e-6f;             // a rejected trial this close (relative) to the accepted cost: the cost is flat to
                                                  // fp32 resolution across the step; a stalled fit is rejected by more

// Orders this wave's LDS accesses: what lanes wrote before is visible to the lanes that read after.  No other wave of the
// workgroup takes part.
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
__device__ inline float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return uniform(v);
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return uniform(v);
}
__device__ inline bool wave_any(bool b) { return __any(b); }
__device__ inline float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// What a pose's wave keeps in registers: wave uniform unless a lane is named.
struct FitState {
  bool warm, mirrored, boxed;
  float sign;                            // determinant of the wrist's linear part
  float lo = 0.f, hi = 0.f;              // lanes 0..19: the angle's box
  float tail = 0.f;                      // lanes 20, 21: angles that do not enter the skinning, copied through
  float init_w = 0.f;                    // lanes 0..11: the start's wrist rows as given
  float wl = 0.f;                        // lanes 0..20: the landmark's scalar weight, 0 = unused
  bool used = false;                     // lanes 0..20
  int n_used;
  float wsum;
  float cx = 0.f, cy = 0.f, cz = 0.f, extent = 0.f;      // weighted centroid and extent of the targets
  bool refused, keep_start;              // keep_start: a refused pose gives back the start it was given
  float cost = 0.f, worst = 0.f;         // of the accepted state
  int iters = 0, status;
  bool fresh = true;                     // the accepted state is newer than the normal matrix
};

// P::load of a cost with scalar weights [n,21] (null: 1): a landmark is used when its weight is positive; false when the
// weight is not a finite number >= 0.
__device__ inline bool fit_scalar_weight(const float* weights, int i, int lane, float& wl, bool& used) {
  if (lane >= 21) return true;
  wl = weights ? weights[(size_t)i * 21 + lane] : 1.f;
  const bool valid = wl >= 0.f && wl <= 3.0e38f;
  used = valid && wl > 0.f;
  return valid;
}

// The forward function of (ang, wrist) into S.local / prefix / frame / p: the weighted cost, and the largest residual of
// a weighted landmark in `worst`.  Called by the whole wave.
template <class Lds>
__device__ inline float fit_eval(Lds& S, const float* ang, const float* wrist, int lane, float& worst) {
  if (lane < 20) {
    const M34 l = joint_local(S.hm + 3 * lane, S.hm + 66 + 3 * lane, ang[lane]);
#pragma unroll
    for (int k = 0; k < 12; ++k) S.local[lane][k] = l.m[k];
  }
  wave_sync();
  if (lane < 6) {
    M34 w;
#pragma unroll
    for (int k = 0; k < 12; ++k) w.m[k] = wrist[k];
    if (lane < 5) {
      finger_chain_with_prefixes(w, S.local, lane, S.prefix, S.frame);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) { S.frame[0][k] = w.m[k]; S.frame[1][k] = w.m[k]; }
    }
  }
  wave_sync();
  float d2 = 0.f, wl = 0.f;
  if (lane < 21) {
    float o[3];
    blend_landmark(S.hm, lane, S.frame, o);
    S.p[lane][0] = o[0]; S.p[lane][1] = o[1]; S.p[lane][2] = o[2];
    wl = S.w[lane];
    if (wl > 0.f) {
      const float rx = o[0] - S.target[lane][0], ry = o[1] - S.target[lane][1], rz = o[2] - S.target[lane][2];
      d2 = rx * rx + ry * ry + rz * rz;
    }
  }
  wave_sync();
  // a NaN must not hide behind fmaxf: the sum carries it
  const float cost = wave_sum(wl * d2);
  worst = sqrtf(wave_max(d2));
  return cost;
}

// exp(hat(v)) without the clamp of so3_exp_map (the wrist increment is the solver's own, not the model's)
__device__ inline void rodrigues(float vx, float vy, float vz, float* r) {
  const float n2 = vx * vx + vy * vy + vz * vz;
  float f1, f2;
  if (n2 < 1e-8f) {
    f1 = 1.f - n2 / 6.f; f2 = 0.5f - n2 / 24.f;
  } else {
    const float th = sqrtf(n2);
    f1 = sinf(th) / th; f2 = (1.f - cosf(th)) / n2;
  }
  r[0] = 1.f - f2 * (vy * vy + vz * vz); r[1] = -f1 * vz + f2 * (vx * vy);     r[2] = f1 * vy + f2 * (vx * vz);
  r[3] = f1 * vz + f2 * (vx * vy);       r[4] = 1.f - f2 * (vx * vx + vz * vz); r[5] = -f1 * vx + f2 * (vy * vz);
  r[6] = -f1 * vy + f2 * (vx * vz);      r[7] = f1 * vx + f2 * (vy * vz);       r[8] = 1.f - f2 * (vx * vx + vy * vy);
}

// ---- start

template <class P, class = void>
struct fit_pivot_from_start : std::false_type {};
template <class P>
struct fit_pivot_from_start<P, std::void_t<decltype(P::PIVOT_FROM_START)>> : std::bool_constant<P::PIVOT_FROM_START> {};

// The weighted centroid and extent of 21 points `q` in LDS: the targets', or the start's landmarks' (PIVOT_FROM_START).
__device__ inline void fit_pivot(const float (*q)[3], int lane, FitState& st) {
  const float wl = st.wl, wsum = st.wsum;
  const float tx = lane < 21 ? q[lane][0] : 0.f, ty = lane < 21 ? q[lane][1] : 0.f, tz = lane < 21 ? q[lane][2] : 0.f;
  const float cx = wave_sum(wl * tx) / wsum, cy = wave_sum(wl * ty) / wsum, cz = wave_sum(wl * tz) / wsum;
  st.extent = sqrtf(wave_sum(wl * ((tx - cx) * (tx - cx) + (ty - cy) * (ty - cy) + (tz - cz) * (tz - cz))) / wsum);
  st.cx = cx; st.cy = cy; st.cz = cz;
}

// The model, the landmarks (P::load, then the targets of used ones: others are never read), the box, the start and the refusal
// rules: a weight, factor or target of a used landmark that is not finite, fewer than three used landmarks.  Then the weighted
// centroid and extent of the targets.
template <class P>
__device__ inline void fit_load(P& prob, typename P::Lds& S, const FitPoseArgs& a, int i, int lane, FitState& st) {
  const int mrow = a.n_models == 1 ? 0 : i;
  st.warm = a.init_ja != nullptr;
  st.mirrored = a.mirror && a.mirror[i] == 1;
  st.sign = st.mirrored ? -1.f : 1.f;
  for (int e = lane; e < 321; e += 64) S.hm[e] = a.hand_model[(size_t)mrow * 321 + e];
  bool bad = !prob.load(S, i, mrow, lane, st.wl, st.used);
  if (lane < 21) {
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if constexpr (!fit_pivot_from_start<P>::value) {
      if (!bad && st.used) {
        const float* t = a.targets + (size_t)i * a.target_stride + 3 * lane;
        tx = t[0]; ty = t[1]; tz = t[2];
        bad = !(fabsf(tx) <= 3.0e38f) || !(fabsf(ty) <= 3.0e38f) || !(fabsf(tz) <= 3.0e38f);
      }
    }
    if (bad) { st.wl = 0.f; st.used = false; }
    S.w[lane] = st.wl;
    S.target[lane][0] = tx; S.target[lane][1] = ty; S.target[lane][2] = tz;
  }
  st.boxed = a.limits != nullptr;
  if (lane < 20) {
    float ang0 = 0.f;
    if (st.boxed) { st.lo = a.limits[(size_t)mrow * 40 + 2 * lane]; st.hi = a.limits[(size_t)mrow * 40 + 2 * lane + 1]; }
    if (st.warm) ang0 = a.init_ja[(size_t)i * a.init_ja_stride + lane];
    if (st.boxed) ang0 = fminf(fmaxf(ang0, st.lo), st.hi);
    S.ang[lane] = ang0;
  }
  if (st.warm && (lane == 20 || lane == 21)) st.tail = a.init_ja[(size_t)i * a.init_ja_stride + lane];
  if (lane < 12) {
    st.init_w = st.warm ? a.init_xf[(size_t)i * a.init_xf_stride + lane] : ((lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f);
    float v = st.init_w;
    if ((lane & 3) == 3) v *= a.t_scale;
    if ((lane & 3) == 0 && st.mirrored) v = -v;
    S.wrist[lane] = v;
  }
  st.n_used = __popcll(__ballot(st.used));
  st.refused = wave_any(bad) || st.n_used < 3;
  st.keep_start = st.warm;
  st.wsum = wave_sum(st.wl);
  wave_sync();
  if constexpr (!fit_pivot_from_start<P>::value) {
    if (!st.refused) fit_pivot(S.target, lane, st);
  }
}

// Cold start: the rest pose (inside the box), aligned to the targets by a weighted Kabsch fit of its landmarks.  H and the
// rotation in fp64 (ut_math.h), every lane the same values.
template <class Lds>
__device__ inline void fit_cold_start(Lds& S, int lane, const FitState& st) {
  const float cx = st.cx, cy = st.cy, cz = st.cz, sign = st.sign;
  float unused;
  fit_eval(S, S.ang, S.wrist, lane, unused);
  const double w = st.wl, inv = 1.0 / (double)st.wsum;
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

// ---- (1)

// J into S.jl - per used landmark the joint, wrist and residual columns scaled by P::row_scale, then P::finish_rows.  Needs
// S.prefix / frame / p of the accepted state.  The first half of fit_linearise, on its own for a caller that wants the rows alone.
template <class P>
__device__ inline void fit_rows(P& prob, typename P::Lds& S, int lane, const FitState& st) {
  constexpr int NP = P::NP, LD = P::LD;
  for (int e = lane; e < 63 * LD; e += 64) S.jl[e] = 0.f;
  if (lane < 20) joint_axis_in_world(S.prefix[lane], S.hm + 3 * lane, S.hm + 66 + 3 * lane, S.omega[lane], S.cw[lane]);
  wave_sync();
  if (st.used) {
    const float sw = prob.row_scale(S, lane), sws = sw * st.sign;
    float* row = S.jl + 3 * lane * LD;            // rows 3 l, 3 l + 1, 3 l + 2
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
      const float scale = sws * we;
      for (int j = 0; j <= m; ++j) {
        const int k = 4 * c + j;
        const float vx = yx - S.cw[k][0], vy = yy - S.cw[k][1], vz = yz - S.cw[k][2];
        const float ox = S.omega[k][0], oy = S.omega[k][1], oz = S.omega[k][2];
        row[k] += scale * (oy * vz - oz * vy);
        row[LD + k] += scale * (oz * vx - ox * vz);
        row[2 * LD + k] += scale * (ox * vy - oy * vx);
      }
    }
    const float px = S.p[lane][0], py = S.p[lane][1], pz = S.p[lane][2];
    const float vx = px - st.cx, vy = py - st.cy, vz = pz - st.cz;
    // wrist rotation about the centroid: -hat(v); translation: I
    row[21] = sw * vz;          row[22] = -sw * vy;
    row[LD + 20] = -sw * vz;    row[LD + 22] = sw * vx;
    row[2 * LD + 20] = sw * vy; row[2 * LD + 21] = -sw * vx;
    row[23] = sw; row[LD + 24] = sw; row[2 * LD + 25] = sw;
    row[NP] = sw * (px - S.target[lane][0]);
    row[LD + NP] = sw * (py - S.target[lane][1]);
    row[2 * LD + NP] = sw * (pz - S.target[lane][2]);
    prob.finish_rows(S, lane, row, sw, px, py, pz);
  }
  wave_sync();
}

// fit_rows, and the lower triangle of [J r]^T [J r] into S.a.
template <class P>
__device__ inline void fit_linearise(P& prob, typename P::Lds& S, int lane, const FitState& st) {
  constexpr int NP = P::NP, LD = P::LD;
  fit_rows(prob, S, lane, st);
  // (NP + 1) (NP + 2) / 2 entries (i, j <= i): 378 are 6 per lane, 406 are 7
  for (int e = lane; e < (NP + 1) * (NP + 2) / 2; e += 64) {
    int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    if (i * (i + 1) / 2 > e) --i;
    if ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    float s = 0.f;
#pragma unroll 9
    for (int r = 0; r < 63; ++r) s = fmaf(S.jl[r * LD + i], S.jl[r * LD + j], s);
    S.a[i][j] = s;
  }
  wave_sync();
}

// Marquardt's D on lane i < NP: the diagonal of J^T J with its floor.
template <int NP, class Lds>
__device__ inline float fit_diag(const Lds& S, int lane) {
  const float d = lane < NP ? S.a[lane][lane] : 0.f;
  return fmaxf(d, FIT_DIAG_FLOOR * wave_max(d));
}

// ---- (2)

// delta = -(A + lambda D)^-1 g on lane i < NP (0 on the others), A the leading NP x NP block of S.a and g its row NP, D_i = diag
// on lane i, LD the row stride of S.jl; false when a pivot is not positive and finite or the solution is not finite.  Lane i
// keeps row i of the matrix in registers: every loop below is fully unrolled, so the row is indexed statically and a value of
// another lane is a v_readlane on a constant lane - the right-looking factorisation and the forward solve touch no LDS at
// all.  The backward solve needs column i on lane i: the factor goes through S.jl once (J is dead by then) and comes back
// transposed.  With SOLVE false the factorisation alone, no LDS traffic beyond reading S.a: `delta` is its last pivot.
template <int NP, int LD, bool SOLVE = true, class Lds>
__device__ inline bool fit_solve(Lds& S, int lane, float lambda, float diag, float& delta) {
  const bool row = lane < NP;
  float a[NP], inv_d[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) a[k] = (row && k <= lane) ? S.a[row ? lane : 0][k] + (k == lane ? lambda * diag : 0.f) : 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float piv = lane_value(a[j], j);
    if (!(piv > 0.f) || !(piv <= 3.0e38f)) return false;
    if (!SOLVE && j == NP - 1) { delta = piv; return true; }
    inv_d[j] = 1.f / sqrtf(piv);
    a[j] *= inv_d[j];                                 // L_ij on lanes i >= j (sqrt(piv) on lane j); unused above the diagonal
#pragma unroll
    for (int k = j + 1; k < NP; ++k) a[k] = fmaf(-a[j], lane_value(a[j], k), a[k]);      // A_ik -= L_ij L_kj, used for i >= k
  }
  float b = row ? -S.a[NP][row ? lane : 0] : 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {                 // L y = -g
    const float y = lane_value(b, j) * inv_d[j];
    if (lane == j) b = y;
    else if (row && lane > j) b = fmaf(-a[j], y, b);
  }
  float* L = S.jl;
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (row && k <= lane) L[lane * LD + k] = a[k];
  wave_sync();
  float c[NP];                                    // c[j] = L_j,lane: column `lane` of the factor
#pragma unroll
  for (int j = 0; j < NP; ++j) c[j] = (row && j > lane) ? L[j * LD + lane] : 0.f;
#pragma unroll
  for (int j = NP - 1; j >= 0; --j) {            // L^T x = y
    const float x = lane_value(b, j) * inv_d[j];
    if (lane == j) b = x;
    else if (lane < j) b = fmaf(-c[j], x, b);
  }
  wave_sync();                                        // the factor is read before anybody reuses S.jl
  delta = b;
  return !wave_any(!(fabsf(b) <= 3.0e38f));
}

// ---- (3)

// The trial angles into S.ang_t, and the trial wrist [E R | E (t - c) + c + dt] into S.wrist_t; whether the angles, the
// rotation and the translation all moved by no more than the step tolerances.
template <class Lds>
__device__ inline bool fit_trial(Lds& S, int lane, float delta, const FitState& st) {
  const float cx = st.cx, cy = st.cy, cz = st.cz;
  float step = 0.f;
  if (lane < 20) {
    float t = S.ang[lane] + delta;
    if (st.boxed) t = fminf(fmaxf(t, st.lo), st.hi);
    S.ang_t[lane] = t;
    step = fabsf(t - S.ang[lane]);
  }
  const float rx = lane_value(delta, 20), ry = lane_value(delta, 21), rz = lane_value(delta, 22);
  const float ux = lane_value(delta, 23), uy = lane_value(delta, 24), uz = lane_value(delta, 25);
  float e[9];
  rodrigues(rx, ry, rz, e);
  if (lane < 3) {                                 // row `lane`
    const float e0 = lane == 0 ? e[0] : (lane == 1 ? e[3] : e[6]), e1 = lane == 0 ? e[1] : (lane == 1 ? e[4] : e[7]),
                e2 = lane == 0 ? e[2] : (lane == 1 ? e[5] : e[8]);
    const float* m = S.wrist;
    S.wrist_t[4 * lane] = e0 * m[0] + e1 * m[4] + e2 * m[8];
    S.wrist_t[4 * lane + 1] = e0 * m[1] + e1 * m[5] + e2 * m[9];
    S.wrist_t[4 * lane + 2] = e0 * m[2] + e1 * m[6] + e2 * m[10];
    const float cl = lane == 0 ? cx : (lane == 1 ? cy : cz), ul = lane == 0 ? ux : (lane == 1 ? uy : uz);
    S.wrist_t[4 * lane + 3] = e0 * (m[3] - cx) + e1 * (m[7] - cy) + e2 * (m[11] - cz) + cl + ul;
  }
  return wave_max(step) <= FIT_STEP_TOL && fmaxf(fabsf(rx), fmaxf(fabsf(ry), fabsf(rz))) <= FIT_STEP_TOL &&
         fmaxf(fabsf(ux), fmaxf(fabsf(uy), fabsf(uz))) <= FIT_STEP_TOL * st.extent;
}

// ---- outputs

// The pose and the wrist.  A refused pose gives back its start - the rest pose at the identity on a cold start, and when the
// start itself is what was refused (its cost is not finite).
template <class Lds>
__device__ inline void fit_store_pose(const Lds& S, const FitPoseArgs& a, int i, int lane, const FitState& st) {
  const bool refused = st.refused, keep_start = st.keep_start;
  if (lane < 22) {
    float v = refused && !keep_start ? 0.f : st.tail;
    if (lane < 20) {
      v = refused ? (keep_start ? a.init_ja[(size_t)i * a.init_ja_stride + lane] : 0.f) : S.ang[lane];
      if (!refused && !st.boxed && fabsf(v) > 3.14159265358979f)
        v -= 6.28318530717959f * ceilf((v - 3.14159265358979f) / 6.28318530717959f);      // into (-pi, pi]
    }
    a.ja[(size_t)i * a.ja_stride + lane] = v;
  }
  if (lane < 12) {
    float v = keep_start ? st.init_w : ((lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f);
    if (!refused) {
      v = S.wrist[lane];
      if ((lane & 3) == 3) v /= a.t_scale;
      if ((lane & 3) == 0 && st.mirrored) v = -v;
    }
    a.xf[(size_t)i * a.xf_stride + lane] = v;
  } else if (lane < 16 && a.xf_stride >= 16) {
    a.xf[(size_t)i * a.xf_stride + lane] = lane == 15 ? 1.f : 0.f;
  }
}

// The four floats every info row starts with: rms = sqrt(cost / denominator), the worst residual, iterations, status.
__device__ inline void fit_store_info(float* o, const FitState& st, float denominator, int status) {
  o[0] = st.refused ? 0.f : sqrtf(st.cost / denominator);
  o[1] = st.refused ? 0.f : st.worst;
  o[2] = (float)st.iters;
  o[3] = (float)status;
}

// ---- the fit of pose i by its wave, in the wave's region S
template <class P>
__device__ inline void fit_pose(P& prob, typename P::Lds& S, const FitPoseArgs& a, int i, int lane) {
  constexpr int NP = P::NP, LD = P::LD;
  FitState st;
  fit_load(prob, S, a, i, lane, st);
  if (!st.refused && !st.warm) fit_cold_start(S, lane, st);
  if (!st.refused) {
    const float iso = fit_eval(S, S.ang, S.wrist, lane, st.worst);
    if constexpr (fit_pivot_from_start<P>::value) fit_pivot(S.p, lane, st);
    st.cost = prob.cost(S, lane, st.used, iso);
    if (!(st.cost <= 3.0e38f)) { st.refused = true; st.keep_start = false; }      // a start that is not finite
  }

  st.status = st.refused ? FIT_REFUSED : 0;
  if (!st.refused) {
    float lambda = FIT_LAMBDA_START, diag = 0.f;
    bool done = false;
    for (; st.iters < a.max_iters && !done;) {
      if (st.fresh) {
        fit_linearise(prob, S, lane, st);
        diag = fit_diag<NP>(S, lane);
        st.fresh = false;
      }
      float delta = 0.f;
      const bool ok = fit_solve<NP, LD>(S, lane, lambda, diag, delta);
      ++st.iters;
      if (!ok) { lambda *= FIT_LAMBDA_UP; continue; }
      const bool moved_little = fit_trial(S, lane, delta, st);
      const bool step_small = prob.trial(S, lane, delta) && moved_little;
      wave_sync();
      float worst_t;
      const float iso_t = fit_eval(S, S.ang_t, S.wrist_t, lane, worst_t);
      const float cost_t = prob.cost(S, lane, st.used, iso_t);
      const float cost = st.cost;
      const bool accept = cost_t < cost;              // false for a NaN; +inf cannot be below a finite cost
      const bool flat = !accept || cost - cost_t <= FIT_DECREASE_TOL * cost;
      const bool stationary = !accept && fabsf(cost_t - cost) <= FIT_FLAT_TOL * cost;      // false for a NaN
      done = (step_small && flat && lambda <= FIT_LAMBDA_CONVERGED_MAX) || stationary;
      if (accept) {
        if (lane < 20) S.ang[lane] = S.ang_t[lane];
        if (lane < 12) S.wrist[lane] = S.wrist_t[lane];
        st.cost = cost_t; st.worst = worst_t;
        prob.keep();
        lambda = fmaxf(lambda * FIT_LAMBDA_DOWN, FIT_LAMBDA_MIN);
        st.fresh = true;
        wave_sync();
      } else {
        lambda *= FIT_LAMBDA_UP;
      }
    }
    st.status = done ? FIT_CONVERGED : FIT_AT_MAX_ITERS;
  }

  fit_store_pose(S, a, i, lane, st);
  prob.report(S, i, lane, st);
}

// ---- the hand's scale as a 27th parameter, written once: fit_scale.hip and fit_views_scale.hip derive their problems from it
//
// Scale s means hand.scaled_hand_model(model, s): the 66 joint and 63 landmark rest coordinates times s in fp32, nothing else.
// sigma = ln s is ordered last, d landmark / d sigma = landmark - wrist translation (the deriving problem's finish_rows writes
// that column), the trial scale is clamp(s exp(d sigma), SCALE_MIN, SCALE_MAX), and a small step also needs |d sigma| <=
// FIT_STEP_TOL.  Every trial writes the region's model again from an unscaled copy of those 129 floats.
constexpr int FITS_P = 3;         // poses (waves) per workgroup
constexpr int FITS_SIGMA = 26;    // column of sigma = ln s

struct FitScaleLds {              // one wave's region
  float hm[321];                  // the pose's packed model at the scale of the last evaluated state
  float rest[129];                // its joint (66) and landmark (63) rest coordinates as given: hm[66..194] = rest * scale
  float local[20][12];            // joint transforms of the last evaluated state
  float prefix[20][12];           // W L0 .. L(j-1) in front of joint 4 f + j
  float frame[17][12];            // skinning frames
  float omega[20][3], cw[20][3];  // joint axes and centres in the world (linearisation)
  float jl[63 * 29];              // J while the normal matrix is formed, then the Cholesky factor L [27][29]
  float a[28][29];                // lower triangle of [J r]^T [J r]: A = J^T J, row 27 = g = J^T r
  float ang[20], ang_t[20];       // accepted and trial angles
  float wrist[12], wrist_t[12];   // accepted and trial wrist frame
  float p[21][3];                 // landmarks of the last evaluated state
  float target[21][3], w[21];     // targets (0 where the weight is 0, or without 3-D targets) and scalar weights, 0 = unused
};
static_assert(sizeof(FitScaleLds) == 16416 && sizeof(FitScaleLds) * FITS_P <= 65536, "a workgroup's static LDS");

struct FitScaleParam {
  bool fixed = false;
  float scale = 1.f, scale_t = 1.f;      // of the accepted and of the trial state

  // The model of the region at scale s: the bits of scaled_hand_model.  Called by the whole wave; the caller syncs.
  __device__ inline void set_scale(FitScaleLds& S, float s, int lane) {
    for (int e = lane; e < 129; e += 64) S.hm[66 + e] = S.rest[e] * s;
  }
  // The unscaled rest coordinates and the start's scale; the model at that scale.  False when the start's scale lies outside the
  // bounds: the pose is refused and its scale is 1.
  __device__ inline bool load_scale(FitScaleLds& S, const float* hand_model, int mrow, const float* init_scale, int scale_mode, int i,
                                    int lane) {
    fixed = scale_mode == FITS_MODE_FIXED;
    for (int e = lane; e < 129; e += 64) S.rest[e] = hand_model[(size_t)mrow * 321 + 66 + e];
    if (init_scale) scale = init_scale[i];
    const bool bad_scale = !(scale >= FITS_SCALE_MIN) || !(scale <= FITS_SCALE_MAX);      // a NaN is neither
    if (bad_scale) scale = 1.f;
    wave_sync();                                      // S.hm is written by other lanes
    set_scale(S, scale, lane);
    return !bad_scale;
  }
  __device__ inline bool trial(FitScaleLds& S, int lane, float delta) {
    // with the sigma column zero the floored diagonal gives d sigma = 0; the fixed scale is kept by construction as well
    const float ds = fixed ? 0.f : lane_value(delta, FITS_SIGMA);
    scale_t = fixed ? scale : fminf(fmaxf(scale * expf(ds), FITS_SCALE_MIN), FITS_SCALE_MAX);
    set_scale(S, scale_t, lane);
    return fabsf(ds) <= FIT_STEP_TOL;
  }
  // The scale information of the accepted state of problem `prob` (the object this is a base of), 0 for a refused pose and a
  // fixed scale: the last pivot of the Cholesky factorisation of A + SCALE_INFO_LAMBDA D, i.e. the Schur complement of sigma;
  // FITS_AT_BOUND into `status`.  After an accepted last trial the region holds that state (model at its scale, frames,
  // landmarks) and the normal matrix is the one before it: linearise once more.  After a rejected one the normal matrix is the
  // accepted state's already, and nothing else is needed.
  template <class P>
  __device__ inline float scale_information(P& prob, FitScaleLds& S, int lane, const FitState& st, int& status) {
    float scale_info = 0.f;
    if (!st.refused && !fixed) {
      if (st.fresh) fit_linearise(prob, S, lane, st);
      float pivot = 0.f;                              // stays 0 when a pivot is not positive and finite
      fit_solve<P::NP, P::LD, false>(S, lane, FITS_SCALE_INFO_LAMBDA, fit_diag<P::NP>(S, lane), pivot);
      scale_info = uniform(pivot);
      if (scale <= FITS_SCALE_MIN || scale >= FITS_SCALE_MAX) status |= FITS_AT_BOUND;
    }
    return scale_info;
  }
};

}  // namespace ut
