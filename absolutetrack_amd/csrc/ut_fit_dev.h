// Device-side pieces shared by the pose fits fit.hip (26 parameters) and fit_scale.hip (27: the hand's scale as well): a
// wave's own LDS ordering and reductions, the forward function on a wave's LDS region, the Cholesky solve with one lane per
// row.  An LDS region type `Lds` has the members fit.hip's FitLds documents (hm, local, prefix, frame, p, w, target, jl, a).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ut_fk.h"

namespace ut {

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

// delta = -(A + lambda D)^-1 g on lane i < NP (0 on the others), A the leading NP x NP block of S.a and g its row NP, LD the
// row stride of S.jl; false when a pivot is not positive and finite or the solution is not finite.  diag: D_i on lane i.  Lane i keeps row i of the matrix in registers: every loop below is fully
// unrolled, so the row is indexed statically and a value of another lane is a v_readlane on a constant lane - the
// right-looking factorisation and the forward solve touch no LDS at all.  The backward solve needs column i on lane i: the
// factor goes through S.jl once (J is dead by then) and comes back transposed.
template <int NP, int LD, class Lds>
__device__ inline bool fit_solve(Lds& S, int lane, float lambda, float diag, float& delta) {
  const bool row = lane < NP;
  float a[NP], inv_d[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) a[k] = (row && k <= lane) ? S.a[row ? lane : 0][k] + (k == lane ? lambda * diag : 0.f) : 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float piv = lane_value(a[j], j);
    if (!(piv > 0.f) || !(piv <= 3.0e38f)) return false;
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

}  // namespace ut
