// Sequences of 2-D detections followed frame by frame in one launch: ut_track_pose_views (include/umetrack_hip_track.h).
// The loop of tracker.track_hand_poses_in_views - warm fit from the previous frame's choice, read the fit's rms back, keep it or
// take the cold chain's row, go on from the choice - moved onto the device: one wave per sequence, FITV_P sequences per workgroup,
// each in its own FitViewsLds region, no workgroup barrier (lengths and iteration counts differ per sequence).  A frame is
// ut_fit_dev.h's fit_pose() on ut_fit_views_dev.h's cost as they are, in a function of its own (track_frame), so a frame's bits are
// those of ut_fit_pose_views_robust on that row from that start; the start is handed over through the output rows themselves:
// frame t reads row t - 1 as its init.
// All tracker state (whether there is a start, the decision) is wave uniform.  The yardstick is the per-frame chain of the existing
// entries (tests/test_gpu_track.py) and tests/track_cases.py in float64.  Registers: DESIGN.md, "Sequences tracked in one launch".
#include "ut_fit_views_dev.h"

namespace ut {
namespace {

// The warm fit of frame t of the wave's sequence: fit_pose() on row i from the start.  NOT inlined into the frame loop, on purpose:
// inlined there, the optimiser sees fit_pose() inside a loop and vectorises and contracts its arithmetic differently from the fit's
// kernels (device assembly: other counts of v_pk_fma_f32 / v_pk_add_f32), and frame 0's rms already differs from ut_fit_pose_views'
// in its last bits.  As a function of its own it compiles to the floating-point instructions of fit_pose_views_kernel /
// fit_pose_views_robust_kernel (equal counts of every kind).  For that it must see what those kernels see: the arguments
// as wave-uniform loads from the kernel's argument segment and not as values in vector registers - the kernel hands over the
// segment's address (its one parameter lies at the start; the builtin that returns the address is null outside a kernel), which
// arrives in vector registers like every argument and is made uniform again here, as the frame number is -, the LDS regions as a
// static array, and a start whose pointer it knows nothing about (it may be null there), so the address goes through an integer.
// Row i of the init resolves to the start: the sequence's own with stride 0 at t = 0, then the previous frame's chosen row.
// The price is the function's frame: DESIGN.md has the scratch bytes and where they are paid.
template <int KIND, int LOSS>
__device__ __attribute__((noinline)) void track_frame(uintptr_t args, int t_in) {
#if defined(__HIP_DEVICE_COMPILE__)                   // the host pass knows no argument segment
  __shared__ FitViewsLds s_all[FITV_P];
  const uintptr_t segment = (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)args) |
                            (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(args >> 32)) << 32;
  const TrackViewsArgs& a = *(const __attribute__((address_space(4))) TrackViewsArgs*)segment;
  const FitViewsArgs& g = a.robust.views;
  const int t = __builtin_amdgcn_readfirstlane(t_in);
  const int seq = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int i = seq * a.n_frames + t;
  FitPoseArgs p = g.pose;
  const bool first = t == 0;
  const uintptr_t ja0 = first ? (uintptr_t)(g.pose.init_ja + (size_t)seq * g.pose.init_ja_stride) : (uintptr_t)g.pose.ja - 4u * (uintptr_t)g.pose.ja_stride;
  const uintptr_t xf0 = first ? (uintptr_t)(g.pose.init_xf + (size_t)seq * g.pose.init_xf_stride) : (uintptr_t)g.pose.xf - 4u * (uintptr_t)g.pose.xf_stride;
  p.init_ja = (const float*)ja0; p.init_ja_stride = first ? 0 : g.pose.ja_stride;
  p.init_xf = (const float*)xf0; p.init_xf_stride = first ? 0 : g.pose.xf_stride;
  FitViewsCost<KIND, LOSS> cost{g};
  cost.c2 = (double)a.robust.loss_scale * (double)a.robust.loss_scale;
  cost.inv_c2 = 1.0 / cost.c2;
  cost.inlier = a.robust.inlier;                      // null, as views.residual is (launch_track_pose_views): read here as the fit's kernel reads it
  fit_pose(cost, s_all[threadIdx.x >> 6], p, i, lane);
#endif
}

// TrackViewsArgs must stay this kernel's ONLY parameter: track_frame reads it at offset 0 of the argument segment.
//
// wave_sync() between a frame's writes and the reads that follow: ut_fit_dev.h documents it for LDS, and here it also orders GLOBAL
// accesses of the wave's own lanes - lane 0's info row read by every lane, the output row read as the next start.  Its fence is
// acquire-release at workgroup scope over all address spaces: the wave's earlier stores are complete (vmcnt(0)) before any later
// load issues, and both go through the one vector L1 of the wave's compute unit, which a store updates, so the load sees them.
// Nothing here is read by another workgroup.
template <int KIND, int LOSS>
__global__ __launch_bounds__(64 * FITV_P, 2) void track_pose_views_kernel(const TrackViewsArgs a) {
  const FitViewsArgs& g = a.robust.views;
  const int seq = blockIdx.x * FITV_P + (threadIdx.x >> 6);
  if (seq >= a.n_seq) return;                         // whole waves leave; nobody waits for them
  const int lane = threadIdx.x & 63;
  const int len = a.lengths ? a.lengths[seq] : a.n_frames;
  if (len < 0 || len > a.n_frames) return;            // a length that means nothing: the sequence writes nothing
  const int row0 = seq * a.n_frames;
  // index check, before the first fit: a row outside [-1, n_rows) in any frame inside the length and the sequence writes nothing
  bool bad_row = false;
  for (int e = lane; e < len * g.max_views; e += 64) {
    const int r = g.cam_rows[(size_t)row0 * g.max_views + e];
    bad_row |= r < -1 || r >= g.n_rows;
  }
  if (wave_any(bad_row)) {
    if (lane == 0) atomicOr(g.status, UT_BAD_SRC_INDEX);
    return;
  }
  // frames at or past the length: no pose, an info row of 0, chosen -1
  for (int e = lane; e < (a.n_frames - len) * 4; e += 64) g.info[(size_t)(row0 + len) * 4 + e] = 0.f;
  for (int e = lane; e < a.n_frames - len; e += 64) a.chosen[row0 + len + e] = -1;

  const bool with_cold = a.cold_ja != nullptr;
  bool have_start = g.pose.init_ja != nullptr;
  for (int t = 0; t < len; ++t) {
    const int i = row0 + t;
    bool take_cold = false;
    int chosen = TRACK_WARM;
    if (have_start) {
      track_frame<KIND, LOSS>((uintptr_t)__builtin_amdgcn_kernarg_segment_ptr(), t);
      wave_sync();                                    // lane 0 wrote the info row: every lane reads it
      if (with_cold) {
        const float rms = g.info[(size_t)i * 4], status = g.info[(size_t)i * 4 + 3];
        // the host loop's comparison in fp64: a rounded product, then a rounded sum - no fused multiply-add
        const double bound = __dadd_rn(__dmul_rn(a.recover_ratio, (double)a.cold_info[(size_t)i * 4]), a.recover_floor);
        const bool lost = ((int)status & FIT_REFUSED) != 0 || (double)rms > bound;
        take_cold = lost && a.cold_index[i] >= 0;
        if (take_cold) chosen = TRACK_COLD;
      }
    } else {                                          // no start yet: with_cold holds (the entry refuses the call otherwise)
      take_cold = true;
      have_start = a.cold_index[i] >= 0;
      chosen = have_start ? TRACK_COLD : TRACK_NONE;
    }
    if (take_cold) {                                  // by the lanes that read the row as the next frame's start
      if (lane < 22) g.pose.ja[(size_t)i * g.pose.ja_stride + lane] = a.cold_ja[(size_t)i * a.cold_ja_stride + lane];
      if (lane < 12) g.pose.xf[(size_t)i * g.pose.xf_stride + lane] = a.cold_xf[(size_t)i * a.cold_xf_stride + lane];
      else if (lane < 16 && g.pose.xf_stride >= 16) g.pose.xf[(size_t)i * g.pose.xf_stride + lane] = lane == 15 ? 1.f : 0.f;
      if (lane < 4) g.info[(size_t)i * 4 + lane] = a.cold_info[(size_t)i * 4 + lane];
    }
    if (lane == 0) a.chosen[i] = chosen;
    wave_sync();                                      // the row is written before the next frame starts from it
  }
}

template <int KIND>
void launch_kind(const TrackViewsArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  if (a.robust.loss == FITV_LOSS_HUBER) hipLaunchKernelGGL((track_pose_views_kernel<KIND, FITV_LOSS_HUBER>), grid, block, 0, s, a);
  else if (a.robust.loss == FITV_LOSS_GEMAN_MCCLURE)
    hipLaunchKernelGGL((track_pose_views_kernel<KIND, FITV_LOSS_GEMAN_MCCLURE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((track_pose_views_kernel<KIND, FITV_LOSS_SQUARED>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_track_pose_views(const TrackViewsArgs& a, hipStream_t s) {
  const FitViewsArgs& g = a.robust.views;
  if (a.n_seq <= 0) return hipSuccess;
  if (g.max_views < 1 || g.max_views > TRI_MAX_VIEWS || a.robust.loss < FITV_LOSS_SQUARED || a.robust.loss > FITV_LOSS_GEMAN_MCCLURE ||
      a.n_frames < 1 || !g.info || !a.chosen || g.residual || a.robust.inlier || (!g.pose.init_ja && !a.cold_ja))
    return hipErrorInvalidValue;
  const dim3 grid((a.n_seq + FITV_P - 1) / FITV_P), block(64 * FITV_P);
  if (g.kind == PROJECT_FISHEYE62) launch_kind<PROJECT_FISHEYE62>(a, grid, block, s);
  else launch_kind<PROJECT_PINHOLE>(a, grid, block, s);
  return hipGetLastError();
}

}  // namespace ut
