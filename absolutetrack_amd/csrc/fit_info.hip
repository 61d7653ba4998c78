// The pose fit on landmarks that come with their information, fp32: ut_fit_pose_info (include/umetrack_hip_info.h).
// Every landmark l brings the lower Cholesky factor L_l of a 3 x 3 information matrix H_l = L_l L_l^T - six floats, what
// ut_triangulate_points_info hands out - and the cost is sum_l |L_l^T (landmark_l - target_l)|^2: one Gauss-Newton
// linearisation of the reprojection cost about the triangulated points.  The yardstick is the float64 restatement in
// tests/info_cases.py.
//
// The solver is ut_fit_dev.h's fit_pose(), on fit.hip's 26 parameters and 63 whitened rows: the three Jacobian rows (and the
// residual column) of a landmark are filled without a weight, and the landmark's lane then replaces the 27 columns
// a = (a0, a1, a2) of its rows by L^T a in place: (l00 a0 + l10 a1 + l20 a2, l11 a1 + l21 a2, l22 a2).  The forward function
// is fit_eval's (ut_fk's arithmetic); its isotropic cost is dropped and the whitened one summed behind it.  A landmark is used
// when any entry of its factor is non-zero; its scalar weight - for the centroid the wrist turns about, the extent and the
// cold start's Kabsch fit - is |L|_F^2 = trace(H).
//
// The factors add 504 bytes to a region: 4 x 15568 = 62272 bytes of the 64 KB a workgroup gets.
#include "ut_fit_dev.h"

namespace ut {
namespace {

constexpr int FITI_P = 4;        // poses (waves) per workgroup

struct FitInfoLds {              // one wave's region, 15568 bytes: FITI_P of them stay inside the 64 KB a workgroup gets
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
  float target[21][3], w[21];    // targets (0 where the landmark is unused) and scalar weights trace(H), 0 = unused
  float li[21][6];               // l00 l10 l11 l20 l21 l22 of every landmark's factor
};
static_assert(sizeof(FitInfoLds) == 15568 && sizeof(FitInfoLds) * FITI_P <= 65536, "a workgroup's static LDS");

struct FitInfoCost {
  using Lds = FitInfoLds;
  static constexpr int NP = 26, LD = 27;
  const FitInfoArgs& a;

  // The factor: used when any entry is non-zero (an unused one is all zeros as it stands), its trace the scalar weight.
  __device__ inline bool load(Lds& S, int i, int, int lane, float& wl, bool& used) {
    if (lane >= 21) return true;
    const float* f = a.sqrt_info + ((size_t)i * 21 + lane) * 6;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float l = f[k];
      bad = bad || !(fabsf(l) <= 3.0e38f);
      used = used || l != 0.f;
      wl = fmaf(l, l, wl);
      S.li[lane][k] = l;
    }
    return !bad && wl <= 3.0e38f;
  }
  __device__ inline float row_scale(const Lds&, int) { return 1.f; }
  // rows <- L^T rows: this lane wrote them, nobody else reads them before the wave_sync that follows
  __device__ inline void finish_rows(Lds& S, int lane, float* row, float, float, float, float) {
    const float l00 = S.li[lane][0], l10 = S.li[lane][1], l11 = S.li[lane][2], l20 = S.li[lane][3], l21 = S.li[lane][4],
                l22 = S.li[lane][5];
    for (int c = 0; c < LD; ++c) {
      const float a0 = row[c], a1 = row[LD + c], a2 = row[2 * LD + c];
      row[c] = l00 * a0 + l10 * a1 + l20 * a2;
      row[LD + c] = l11 * a1 + l21 * a2;
      row[2 * LD + c] = l22 * a2;
    }
  }
  // The whitened cost sum_l |L_l^T (p_l - target_l)|^2 of the state fit_eval left in S.p.
  __device__ inline float cost(const Lds& S, int lane, bool used, float) {
    float c = 0.f;
    if (used) {
      const float* l = S.li[lane];
      const float r0 = S.p[lane][0] - S.target[lane][0], r1 = S.p[lane][1] - S.target[lane][1], r2 = S.p[lane][2] - S.target[lane][2];
      const float u0 = l[0] * r0 + l[1] * r1 + l[3] * r2, u1 = l[2] * r1 + l[4] * r2, u2 = l[5] * r2;
      c = u0 * u0 + u1 * u1 + u2 * u2;
    }
    return wave_sum(c);               // carries a NaN of the state
  }
  __device__ inline bool trial(Lds&, int, float) { return true; }
  __device__ inline void keep() {}
  // rms over the 3 n_used whitened residuals
  __device__ inline void report(Lds&, int i, int lane, const FitState& st) {
    if (a.info && lane == 0) fit_store_info(a.info + (size_t)i * 4, st, (float)(3 * st.n_used), st.status);
  }
};

__global__ __launch_bounds__(64 * FITI_P) void fit_pose_info_kernel(const FitInfoArgs a) {
  __shared__ FitInfoLds s_all[FITI_P];
  const int i = blockIdx.x * FITI_P + (threadIdx.x >> 6);
  if (i >= a.pose.n) return;                          // whole waves leave; nobody waits for them
  FitInfoCost cost{a};
  fit_pose(cost, s_all[threadIdx.x >> 6], a.pose, i, threadIdx.x & 63);
}

}  // namespace

hipError_t launch_fit_pose_info(const FitInfoArgs& a, hipStream_t s) {
  if (a.pose.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fit_pose_info_kernel, dim3((a.pose.n + FITI_P - 1) / FITI_P), dim3(64 * FITI_P), 0, s, a);
  return hipGetLastError();
}

}  // namespace ut
