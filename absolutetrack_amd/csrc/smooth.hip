// Fitted poses smoothed over a sequence: ut_smooth_pose_sequence (include/umetrack_hip_smooth.h, which states the model).  The
// yardstick is the float64 dense solve in tests/smooth_cases.py.
//
// One wave per sequence, SM_P sequences per workgroup, frames in order, no workgroup barrier, every branch wave uniform.  The
// pattern is fit_solve's (ut_fit_dev.h): lane i < 26 keeps row i of a symmetric 26 x 26 matrix in registers, every loop over the
// row is fully unrolled, a value of another lane is a v_readlane on a constant lane.
//  forward   P (rows in registers) and eta (lane i: entry i) of the information filter.  Per step: S = P + W scaled to unit
//            diagonal and factorised in registers (sm_factor, the pivot rule of pose_info_views.hip); the factor of S itself stays
//            in registers, row j on lane j, and goes to the frame's workspace row.  Then every lane solves S x = b for a right-hand
//            side of its own, in place, an entry of the factor a v_readlane into a scalar operand: lane i < 26 column i of P (its
//            own row: P is symmetric), lane 26 the vector eta - P d.  W x is column i of M = W S^-1 P - the product form - and
//            eta's successor; M is symmetrised through one transposition in LDS, then H' of the frame is added.
//  backward  from the last frame: the factor of P_T-1 (SINGULAR when a pivot fails), then per frame the factor of S_t back from the
//            workspace (lane j its own row); lane 26 solves for u_t, lanes < 26 run C_t = L^-T (I + L^-1 W C_t+1 W L^-T) L^-1 in
//            place as forward, transpose, forward, + I, backward, transpose, backward.  The frame's pose is read again, corrected
//            and written: a frame is read before it is written, so the outputs may be the inputs' own buffers.
// Workspace row of frame t: the factor of S_t packed like pose_info (1 / L_ii on the diagonal), eta_t, d_t, a_t, the smallest
// pivot, the weight in force (0 for a gap).  Registers and scratch: DESIGN.md, "Poses smoothed over a sequence".
#include "ut_fit_dev.h"

namespace ut {
namespace {

constexpr int SM_NP = 26, SM_LD = 27, SM_P = 4;
constexpr int SM_ETA = 351, SM_D = 377, SM_A = 403, SM_PIV = 406, SM_F = 407;
static_assert(SM_F + 1 == SMOOTH_WORK, "the workspace row");
constexpr float SM_PI = 3.14159265358979f, SM_2PI = 6.28318530717959f;

struct SmoothLds {                // one wave's region
  float t[SM_NP * SM_LD];         // transpositions: the row stride is odd, so that lanes reading one column hit distinct banks
};

__device__ inline bool sm_finite(float v) { return fabsf(v) <= 3.0e38f; }
__device__ inline float sm_wrap(float v) {            // into (-pi, pi], as fit_store_pose
  if (fabsf(v) > SM_PI) v -= SM_2PI * ceilf((v - SM_PI) / SM_2PI);
  return v;
}

// Row `lane` of a symmetric matrix in m[] (entries k <= lane are read) + diag(add) = M: D^-1/2 M D^-1/2 factorised as cov_factor of
// pose_info_views.hip does, then row `lane` of L' = D^1/2 L, the factor of M itself, in a[] (1 / L'_ii on the diagonal, 0 above
// it and on lanes >= 26).  min_pivot: the smallest pivot up to and including the first one that failed; false when a diagonal
// entry is not positive and finite or a pivot is <= COV_MIN_PIVOT.
__device__ inline bool sm_factor(int lane, const float (&m)[SM_NP], float add, float (&a)[SM_NP], float& min_pivot) {
  constexpr int NP = SM_NP;
  const bool row = lane < NP;
  float d = 1.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) d = k == lane ? m[k] + add : d;
  const bool has = d > 0.f && d <= 3.0e38f;
  const float sd = has ? sqrtf(d) : 0.f;
  const float s = has ? 1.f / sd : 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const float sk = lane_value(s, k);
    a[k] = (row && k < lane) ? m[k] * s * sk : ((row && k == lane && has) ? 1.f : 0.f);
  }
  min_pivot = 1.f;
  bool alive = true;                                  // straight-line: after a failed pivot the rest runs on 1 and is thrown away
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float piv = lane_value(a[j], j);
    const bool good = piv > COV_MIN_PIVOT && piv <= 3.0e38f;
    min_pivot = alive ? fminf(min_pivot, good ? piv : fmaxf(piv, 0.f)) : min_pivot;      // fmaxf drops a NaN: 0
    alive = alive && good;
    const float inv = good ? 1.f / sqrtf(piv) : 1.f;
    a[j] *= inv;
#pragma unroll
    for (int k = j + 1; k < NP; ++k) a[k] = fmaf(-a[j], lane_value(a[j], k), a[k]);
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) a[k] = !row || k > lane ? 0.f : (k < lane ? a[k] * sd : 1.f / (a[k] * sd));
  return alive;
}

// L y = b and L^T x = y in place: every lane its own right-hand side, lane j row j of the factor in l[] (1 / L_jj on the
// diagonal), an entry of it a v_readlane into a scalar operand.
__device__ inline void sm_forward(const float (&l)[SM_NP], float (&b)[SM_NP]) {
#pragma unroll
  for (int j = 0; j < SM_NP; ++j) {
    float t = b[j];
#pragma unroll
    for (int k = 0; k < j; ++k) t = fmaf(-lane_value(l[k], j), b[k], t);
    b[j] = t * lane_value(l[j], j);
  }
}
__device__ inline void sm_backward(const float (&l)[SM_NP], float (&b)[SM_NP]) {
#pragma unroll
  for (int j = SM_NP - 1; j >= 0; --j) {
    float t = b[j];
#pragma unroll
    for (int k = j + 1; k < SM_NP; ++k) t = fmaf(-lane_value(l[j], k), b[k], t);
    b[j] = t * lane_value(l[j], j);
  }
}

// Lane i < 26 holds column i of a matrix: afterwards row i (SYM false) or row i of its symmetric part (SYM true).  Other lanes
// keep what they have.
template <bool SYM>
__device__ inline void sm_transpose(SmoothLds& S, int lane, float (&v)[SM_NP]) {
  wave_sync();
  if (lane < SM_NP) {
#pragma unroll
    for (int k = 0; k < SM_NP; ++k) S.t[lane * SM_LD + k] = v[k];
  }
  wave_sync();
  if (lane < SM_NP) {
#pragma unroll
    for (int k = 0; k < SM_NP; ++k) v[k] = SYM ? 0.5f * (v[k] + S.t[k * SM_LD + lane]) : S.t[k * SM_LD + lane];
  }
}

// Entry k of lane 26's array on lane k.
__device__ inline float sm_from_lane26(const float (&x)[SM_NP], int lane) {
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < SM_NP; ++k) {
    const float v = lane_value(x[k], 26);
    r = lane == k ? v : r;
  }
  return r;
}

// A frame's pose: wave uniform but for `ang`.
struct SmPose {
  float ang;                      // lanes 0..21
  float m[12];                    // the wrist rows as stored, the translation in target units
  float x[3];                     // the body point in the world
  bool finite;
};

__device__ inline SmPose sm_load_pose(const SmoothArgs& a, size_t r, int lane, const float (&b)[3]) {
  SmPose p;
  p.ang = lane < 22 ? a.ja[r * a.ja_stride + lane] : 0.f;
  const float w = lane < 12 ? a.xf[r * a.xf_stride + lane] : 0.f;
#pragma unroll
  for (int k = 0; k < 12; ++k) p.m[k] = lane_value(w, k) * ((k & 3) == 3 ? a.t_scale : 1.f);
  const float* m = p.m;
  const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
  const float bx = det < 0.f ? -b[0] : b[0];          // b is given in the proper wrist frame
#pragma unroll
  for (int k = 0; k < 3; ++k) p.x[k] = m[4 * k] * bx + m[4 * k + 1] * b[1] + m[4 * k + 2] * b[2] + m[4 * k + 3];
  p.finite = !wave_any(!sm_finite(p.ang) || !sm_finite(w)) && sm_finite(p.x[0]) && sm_finite(p.x[1]) && sm_finite(p.x[2]);
  return p;
}

// d on lane i: the fitted step from p to q.
__device__ inline float sm_step(const SmPose& p, const SmPose& q, int lane) {
  float r[9];                                         // Q = R_q R_p^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = q.m[4 * i] * p.m[4 * j] + q.m[4 * i + 1] * p.m[4 * j + 1] + q.m[4 * i + 2] * p.m[4 * j + 2];
  const float vx = 0.5f * (r[7] - r[5]), vy = 0.5f * (r[2] - r[6]), vz = 0.5f * (r[3] - r[1]);
  const float s2 = vx * vx + vy * vy + vz * vz, s = sqrtf(s2), c = 0.5f * (r[0] + r[4] + r[8] - 1.f);
  const float g = s < 1e-4f ? 1.f + s2 / 6.f : atan2f(s, c) / s;      // theta / sin(theta); loses accuracy as theta nears pi
  float d = sm_wrap(q.ang - p.ang);
  d = lane == 20 ? g * vx : (lane == 21 ? g * vy : (lane == 22 ? g * vz : d));
  d = lane == 23 ? q.x[0] - p.x[0] : (lane == 24 ? q.x[1] - p.x[1] : (lane == 25 ? q.x[2] - p.x[2] : d));
  return lane < SM_NP ? d : 0.f;
}

// Row `lane` of H out of the packed triangle; whether an entry is not finite, whether all are 0.
__device__ inline void sm_load_info(const float* hp, int lane, float (&h)[SM_NP], bool& bad, bool& zero) {
  bool b = false, nz = false;
  const int ln = lane < SM_NP ? lane : 0;             // every lane loads: no branch per entry
#pragma unroll
  for (int k = 0; k < SM_NP; ++k) {
    const int i = ln > k ? ln : k, j = ln > k ? k : ln;
    h[k] = lane < SM_NP ? hp[i * (i + 1) / 2 + j] : 0.f;
    b |= !sm_finite(h[k]);
    nz |= h[k] != 0.f;
  }
  bad = wave_any(b);
  zero = !wave_any(nz);
}

// Row `lane` of f B^-T H B^-1, B^-1 = I + [a]x in the block (rows 23..25, columns 20..22).
__device__ inline void sm_repivot(float (&h)[SM_NP], const float (&a)[3], float f, int lane) {
  const float ax = a[0], ay = a[1], az = a[2];
  const float c0 = h[24] * az - h[25] * ay, c1 = h[25] * ax - h[23] * az, c2 = h[23] * ay - h[24] * ax;
  h[20] += c0; h[21] += c1; h[22] += c2;
#pragma unroll
  for (int k = 0; k < SM_NP; ++k) {
    const float g0 = lane_value(h[k], 23), g1 = lane_value(h[k], 24), g2 = lane_value(h[k], 25);
    const float add = lane == 20 ? g1 * az - g2 * ay : (lane == 21 ? g2 * ax - g0 * az : (lane == 22 ? g0 * ay - g1 * ax : 0.f));
    h[k] = (h[k] + add) * f;
  }
}

__device__ inline void sm_copy_frame(const SmoothArgs& a, size_t r, int lane) {
  if (lane < 22) a.ja_out[r * a.ja_out_stride + lane] = a.ja[r * a.ja_stride + lane];
  if (lane < 12) a.xf_out[r * a.xf_out_stride + lane] = a.xf[r * a.xf_stride + lane];
  else if (lane < 16 && a.xf_out_stride >= 16) a.xf_out[r * a.xf_out_stride + lane] = lane == 15 ? 1.f : 0.f;
}

template <bool SIGMA>
__global__ __launch_bounds__(64 * SM_P, 2) void smooth_pose_sequence_kernel(const SmoothArgs a) {
  constexpr int NP = SM_NP;
  __shared__ SmoothLds s_all[SM_P];
  const int seq = blockIdx.x * SM_P + (threadIdx.x >> 6);
  if (seq >= a.n_seq) return;                         // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  SmoothLds& S = s_all[threadIdx.x >> 6];
  const int T = a.n_frames;
  const size_t base = (size_t)seq * T;

  int len = a.lengths ? a.lengths[seq] : T;
  bool refused = len < 0 || len > T;
  if (refused) len = 0;
  const float qv = lane < NP ? a.step_var[(size_t)(a.n_var == 1 ? 0 : seq) * NP + lane] : 1.f;
  const float wl = lane < NP ? 1.f / qv : 0.f;
  if (wave_any(!(qv > 0.f) || !(qv <= 3.0e38f) || !(wl <= 3.0e38f))) refused = true;
  float b3[3] = {0.f, 0.f, 0.f};
  if (a.centre) { b3[0] = a.centre[(size_t)seq * 3]; b3[1] = a.centre[(size_t)seq * 3 + 1]; b3[2] = a.centre[(size_t)seq * 3 + 2]; }

  // ---- forward: P is solved in place, so that a step keeps one matrix in registers
  float P[NP], eta = 0.f, last_pivot = 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) P[k] = 0.f;
  bool singular = false, complete = true;             // complete: every frame inside the length has its workspace row
  for (int t = 0; t < len && !refused && !singular; ++t) {
    const size_t r = base + t;
    float* wp = a.workspace + r * SMOOTH_WORK;
    const SmPose cur = sm_load_pose(a, r, lane, b3);
    float f = a.frame_weight ? a.frame_weight[r] : 1.f;
    if (!cur.finite || !(f >= 0.f) || !(f <= 3.0e38f)) { refused = true; break; }
    if (t > 0) {
      float* wq = wp - SMOOTH_WORK;                   // the row of frame t - 1
      const float d = sm_step(sm_load_pose(a, r - 1, lane, b3), cur, lane);
      float L[NP], min_pivot;
      if (!sm_factor(lane, P, wl, L, min_pivot)) { singular = true; complete = false; break; }      // S is positive definite: overflow only
      if (lane < NP) {
#pragma unroll
        for (int k = 0; k < NP; ++k)
          if (k <= lane) wq[lane * (lane + 1) / 2 + k] = L[k];
        wq[SM_ETA + lane] = eta;
        wq[SM_D + lane] = d;
      }
      if (lane == 0) wq[SM_PIV] = min_pivot;
      float rhs = eta;                                // eta - P d
#pragma unroll
      for (int k = 0; k < NP; ++k) rhs = fmaf(-P[k], lane_value(d, k), rhs);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const float rk = lane_value(rhs, k);
        P[k] = lane < NP ? P[k] : (lane == 26 ? rk : 0.f);
      }
      sm_forward(L, P);
      sm_backward(L, P);
#pragma unroll
      for (int k = 0; k < NP; ++k) P[k] *= lane_value(wl, k);      // lane i: column i of W S^-1 P; lane 26: eta's successor
      eta = sm_from_lane26(P, lane);
      sm_transpose<true>(S, lane, P);
    }
    float av[3] = {0.f, 0.f, 0.f};
    if (f > 0.f) {
      const float* c = a.pivot + r * 3;
      const float cx = c[0], cy = c[1], cz = c[2];
      float h[NP];
      bool bad, zero;
      sm_load_info(a.pose_info + r * 351, lane, h, bad, zero);
      if (bad || !sm_finite(cx) || !sm_finite(cy) || !sm_finite(cz)) { refused = true; break; }
      if (zero) f = 0.f;
      else {
        av[0] = cur.x[0] - cx; av[1] = cur.x[1] - cy; av[2] = cur.x[2] - cz;
        sm_repivot(h, av, f, lane);
#pragma unroll
        for (int k = 0; k < NP; ++k) P[k] = lane < NP ? P[k] + h[k] : 0.f;
      }
    }
    if (lane < 3) wp[SM_A + lane] = lane == 0 ? av[0] : (lane == 1 ? av[1] : av[2]);
    if (lane == 3) wp[SM_F] = f;
  }

  float L[NP];                                        // the factor in force in the backward pass, first P_T-1's
  if (!refused && !singular && len > 0) singular = !sm_factor(lane, P, 0.f, L, last_pivot);
  __threadfence();                                    // lanes read workspace entries that other lanes of the wave wrote

  // ---- frames that are copied through
  float* o_sigma = a.param_sigma;
  float* o_info = a.info;
  const bool through = refused || singular;
  for (int t = through ? 0 : len; t < T; ++t) {
    const size_t r = base + t;
    const bool inside = t < len;                      // only a singular sequence has such frames here
    sm_copy_frame(a, r, lane);
    if (o_sigma && lane < NP) o_sigma[r * NP + lane] = (inside && singular) ? INFINITY : 0.f;
    if (o_info && lane < 4) {
      const float piv = (inside && singular && complete) ? (t == len - 1 ? last_pivot : a.workspace[r * SMOOTH_WORK + SM_PIV]) : 0.f;
      const float status = refused ? (float)SMOOTH_REFUSED : (inside ? (float)SMOOTH_SINGULAR : 0.f);
      o_info[r * 4 + lane] = lane == 2 ? piv : (lane == 3 ? status : 0.f);
    }
  }
  if (through) return;

  // ---- backward
  float C[NP], u_next = 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) C[k] = 0.f;
  for (int t = len - 1; t >= 0; --t) {
    const size_t r = base + t;
    const float* wp = a.workspace + r * SMOOTH_WORK;
    float d = 0.f, min_pivot = last_pivot;
    if (t < len - 1) {
      const int ln = lane < NP ? lane : 0;
#pragma unroll
      for (int k = 0; k < NP; ++k) L[k] = (lane < NP && k <= lane) ? wp[ln * (ln + 1) / 2 + (k <= ln ? k : 0)] : 0.f;
      eta = lane < NP ? wp[SM_ETA + ln] : 0.f;
      d = lane < NP ? wp[SM_D + ln] : 0.f;
      min_pivot = wp[SM_PIV];
    }
    const float rhs = lane < NP ? eta + wl * (u_next + d) : 0.f;
    if constexpr (SIGMA) {                            // C in place; lane 26 carries 0 through the first half
#pragma unroll
      for (int k = 0; k < NP; ++k) C[k] = lane < NP ? lane_value(wl, k) * C[k] * wl : 0.f;
      sm_forward(L, C);
      sm_transpose<false>(S, lane, C);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const float rk = lane_value(rhs, k);
      C[k] = lane == 26 ? rk : (SIGMA ? C[k] : 0.f);
    }
    sm_forward(L, C);
    if constexpr (SIGMA) {
#pragma unroll
      for (int k = 0; k < NP; ++k) C[k] += k == lane ? 1.f : 0.f;
    }
    sm_backward(L, C);
    const float u = sm_from_lane26(C, lane);
    float var = 0.f;
    if constexpr (SIGMA) {
      sm_transpose<false>(S, lane, C);
#pragma unroll
      for (int k = 0; k < NP; ++k) C[k] = lane < NP ? C[k] : 0.f;
      sm_backward(L, C);
      sm_transpose<true>(S, lane, C);                 // symmetrise: the diagonal is untouched
#pragma unroll
      for (int k = 0; k < NP; ++k) var = k == lane ? C[k] : var;
    }

    // the frame's pose again, its correction, its figures
    const SmPose cur = sm_load_pose(a, r, lane, b3);
    const float f = wp[SM_F];
    const float av[3] = {wp[SM_A], wp[SM_A + 1], wp[SM_A + 2]};
    float moved = 0.f;
    if (f > 0.f) {
      float h[NP];
      bool bad, zero;
      sm_load_info(a.pose_info + r * 351, lane, h, bad, zero);
      sm_repivot(h, av, f, lane);
      float hu = 0.f;
#pragma unroll
      for (int k = 0; k < NP; ++k) hu = fmaf(h[k], lane_value(u, k), hu);
      moved = sqrtf(fmaxf(wave_sum(lane < NP ? u * hu : 0.f), 0.f));
    }
    const float mt = t < len - 1 ? d + u_next - u : 0.f;
    const float stepped = sqrtf(wave_sum(lane < NP ? wl * mt * mt : 0.f));
    const float ox = lane_value(u, 20), oy = lane_value(u, 21), oz = lane_value(u, 22);
    // delta = B^-1 u: tau = u_tau + a x omega
    const float tx = lane_value(u, 23) + av[1] * oz - av[2] * oy, ty = lane_value(u, 24) + av[2] * ox - av[0] * oz,
                tz = lane_value(u, 25) + av[0] * oy - av[1] * ox;
    const float cx = cur.x[0] - av[0], cy = cur.x[1] - av[1], cz = cur.x[2] - av[2];
    float e[9];
    rodrigues(ox, oy, oz, e);
    const float* m = cur.m;
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float e0 = e[3 * i], e1 = e[3 * i + 1], e2 = e[3 * i + 2];
      const float cl = i == 0 ? cx : (i == 1 ? cy : cz), tl = i == 0 ? tx : (i == 1 ? ty : tz);
      const float v0 = e0 * m[0] + e1 * m[4] + e2 * m[8], v1 = e0 * m[1] + e1 * m[5] + e2 * m[9], v2 = e0 * m[2] + e1 * m[6] + e2 * m[10];
      const float v3 = (e0 * (m[3] - cx) + e1 * (m[7] - cy) + e2 * (m[11] - cz) + cl + tl) / a.t_scale;
      out = lane == 4 * i ? v0 : (lane == 4 * i + 1 ? v1 : (lane == 4 * i + 2 ? v2 : (lane == 4 * i + 3 ? v3 : out)));
    }
    if (lane < 22) a.ja_out[r * a.ja_out_stride + lane] = lane < 20 ? sm_wrap(cur.ang + u) : cur.ang;
    if (lane < 12) a.xf_out[r * a.xf_out_stride + lane] = out;
    else if (lane < 16 && a.xf_out_stride >= 16) a.xf_out[r * a.xf_out_stride + lane] = lane == 15 ? 1.f : 0.f;
    if constexpr (SIGMA) {
      if (lane < NP) o_sigma[r * NP + lane] = sqrtf(var);
    }
    if (o_info && lane < 4) {
      const float status = (float)(SMOOTH_OK | (f > 0.f ? 0 : SMOOTH_GAP));
      o_info[r * 4 + lane] = lane == 0 ? moved : (lane == 1 ? stepped : (lane == 2 ? min_pivot : status));
    }
    u_next = u;
  }
}

}  // namespace

hipError_t launch_smooth_pose_sequence(const SmoothArgs& a, hipStream_t s) {
  if (a.n_seq <= 0) return hipSuccess;
  if (a.n_frames < 1 || !a.ja || !a.xf || !a.pose_info || !a.pivot || !a.step_var || !a.workspace || !a.ja_out || !a.xf_out)
    return hipErrorInvalidValue;
  const dim3 grid((a.n_seq + SM_P - 1) / SM_P), block(64 * SM_P);
  if (a.param_sigma) hipLaunchKernelGGL(smooth_pose_sequence_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(smooth_pose_sequence_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
