// Streaming 1x1 convolutions on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32): the shortcut convolution of layer4, the
// projection, and the head's two chains (fusion 144 -> 108 -> 72 -> 72, temporal 90 -> 90 x 3) as one launch each.
//
// conv_igemm.hip is built for long K: these layers have 2 .. 8 chunks of K per tile, so its tile prologue, first-touch latency and
// epilogue dominate each launch, and its 128-wide N tile multiplies zeros for the 72-channel layers.  Here a WAVE owns 32 output
// pixels and no operand is shared between waves: after one barrier behind the staging of the biases in LDS the waves run on their
// own - no operand in LDS, no barrier in the loop, no tile queue (every tile costs the same: tiles are dealt round-robin over the
// waves of the grid).
//
// Same bits as conv_igemm.  The operand roles are conv_igemm's (weights = MFMA "A", pixels = "B"), so is the order of K (chunk of
// 32 ascending, q = 0 .. 3, then the four floats of the lane's 16-byte run) and the accumulator's initial value (bias + 0): every
// accumulator sees the same fma chain.  In MFMA step (chunk j, q, c) lane (fr = lane & 31, fh = lane >> 5) supplies pixel fr at
// k = 32 j + 8 q + 4 fh + c; in the accumulator layout the same lane holds pixel fr, and register 4 g + c of 32-channel block j is
// output channel 32 j + 8 g + 4 fh + c.  The two are the same map with q = g: after max(., 0) the accumulators of one layer ARE the
// B operands of the next 1x1 layer, in place - a chain runs in registers and its intermediates never reach memory.  Padded
// channels need no special case: zero weight rows and a zero bias give exact zeros, and the next layer's k_pad is 32 x (blocks of
// this one).  The first layer reads k_pad floats from its pixel's first channel whatever cin is (the run behind cin meets zero
// weights), as conv_igemm's gather does.
//
// Layer-0 pixels and all weights come straight from global memory / L2 into registers, as 16-byte loads ahead of their MFMAs; a
// step (8 k) is 4 x (cout blocks) MFMAs = 768 .. 1024 matrix-pipe cycles.  The biases sit in LDS (staged once per workgroup).
//  * Weights: two steps ahead, from a copy of the packed matrix in FRAGMENT ORDER (PackedConv::wfrag: what the 64 lanes of a step
//    consume is one contiguous kilobyte).  Read from the row-major matrix a lane's 16 bytes are a quarter of a 128-byte line of its
//    own row: every load touched 32 lines and every line came in four times, and at 168 KB of weights per chain against a 32 KB L1
//    that was four L2 reads per line - the L1 fill rate of a CU, not the matrix pipe, set the pace (fusion chain 117 us; the first
//    measurements are in DESIGN.md).
//  * Pixels: a lane reads 16 bytes of ITS pixel per step, so the same quarter-line pattern is inherent; the four loads of a 32-wide
//    chunk are issued together, one chunk ahead, so that the three later ones meet the line the first one brought in.
//  * The request stream runs across tiles: a tile's last chunk asks for the next tile's first pixels and weights (pw_layer_in), in
//    front of this tile's stores.
//  * Layer4's shortcut is memory bound: it takes two cout blocks at a time, in passes over the tile's pixels (the later passes
//    find them in cache), which fits four waves per SIMD (UT_PW_SHAPES).
#include "ut_kernels.h"
#include "ut_conv_dev.h"

namespace ut {

namespace {

constexpr unsigned PW_OOB = 0x80000000u;   // beyond every descriptor (sizes are checked below 2^31), and stays so + a few KB

__device__ __forceinline__ float4 pw_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// weights: always in range, so the fragment's position can sit in the instruction's scalar offset (which the descriptor's range
// check does not cover) and every load of a lane shares ONE address register
__device__ __forceinline__ float4 pw_load4w(__amdgpu_buffer_rsrc_t r, unsigned lane_off, unsigned frag_off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, frag_off, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// accumulators := the layer's bias (+ 0 as conv_igemm adds its empty residual, done once when the bias is staged), from LDS: LDS
// reads have their own counter, a global load here would queue behind the previous tile's stores
template <int NB>
__device__ __forceinline__ void pw_init(f32x16 (&acc)[NB], const float* bias_s /* LDS, the first block's */, int fh) {
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b = *reinterpret_cast<const float4*>(bias_s + 32 * n + 8 * g + 4 * fh);
      acc[n][4 * g + 0] = b.x; acc[n][4 * g + 1] = b.y; acc[n][4 * g + 2] = b.z; acc[n][4 * g + 3] = b.w;
    }
}

#define PW_MFMA_STEP(ACC, WC, B)                                                                                      \
  _Pragma("unroll") for (int n = 0; n < NB; ++n) ACC[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(WC[n].x, B.x, ACC[n], 0, 0, 0); \
  _Pragma("unroll") for (int n = 0; n < NB; ++n) ACC[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(WC[n].y, B.y, ACC[n], 0, 0, 0); \
  _Pragma("unroll") for (int n = 0; n < NB; ++n) ACC[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(WC[n].z, B.z, ACC[n], 0, 0, 0); \
  _Pragma("unroll") for (int n = 0; n < NB; ++n) ACC[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(WC[n].w, B.w, ACC[n], 0, 0, 0);

// Layer 0 of a unit of work (a tile, or one pass over a tile) over NS = k_pad / 8 steps.  w_lane: the lane's 16 bytes of a fragment;
// w_base (wave-uniform): the unit's first fragment in the fragment-ordered weights (step s is 1 KB further, block n NS KB).  The
// pixels come from `in` at in_off + 32 s bytes, the four steps of a chunk together and a chunk ahead; the weights two steps
// ahead.  The stream does not stop at the unit's end: its last chunk requests the NEXT unit's first chunk (in_off_next) and its
// last two steps the next unit's first two weight steps (w_base_next), so those are under way before this unit's stores are issued
// (memory operations complete in order: a load behind the stores waits for them) and a unit never starts with a cold request.
// bfirst / wfirst: this unit's first chunk and first two weight steps on entry, the next unit's on exit.
// The cout blocks are visited round-robin: consecutive MFMAs are independent.  The scheduling barriers keep the requests in front
// of a step's MFMAs; the waits are the compiler's.
template <int NB, int NS>
__device__ __forceinline__ void pw_layer_in(f32x16 (&acc)[NB], __amdgpu_buffer_rsrc_t w_rsrc, unsigned w_lane, unsigned w_base,
                                            unsigned w_base_next, __amdgpu_buffer_rsrc_t in_rsrc, unsigned in_off,
                                            unsigned in_off_next, float4 (&bfirst)[4], float4 (&wfirst)[2][NB]) {
  static_assert(NS % 4 == 0 && NS >= 4, "whole chunks");
  float4 wr[2][NB], br[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < NB; ++n) wr[i][n] = wfirst[i][n];
#pragma unroll
  for (int q = 0; q < 4; ++q) br[0][q] = bfirst[q];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float4 wc[NB];
    if ((s & 3) == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        br[((s >> 2) + 1) & 1][q] = s + 4 < NS ? pw_load4(in_rsrc, in_off + 32 * (s + 4 + q)) : pw_load4(in_rsrc, in_off_next + 32 * q);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) wc[n] = wr[s & 1][n];
    const float4 b = br[(s >> 2) & 1][s & 3];
#pragma unroll
    for (int n = 0; n < NB; ++n)
      wr[s & 1][n] = s + 2 < NS ? pw_load4w(w_rsrc, w_lane, w_base + (unsigned)(n * NS + s + 2) * 1024u)
                                : pw_load4w(w_rsrc, w_lane, w_base_next + (unsigned)(n * NS + s + 2 - NS) * 1024u);
    __builtin_amdgcn_sched_barrier(0);
    PW_MFMA_STEP(acc, wc, b)
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < NB; ++n) wfirst[i][n] = wr[i][n];          // (NS is even: step NS + i sits in wr[i])
#pragma unroll
  for (int q = 0; q < 4; ++q) bfirst[q] = br[(NS >> 2) & 1][q];
}

// A later layer of a chain: the B operand of step s = 4 j + q is max(prev[j][4 q .. 4 q + 3], floor), the previous layer's
// accumulators where they stand.  Weights two steps ahead.
template <int NB, int NS, int NP>
__device__ __forceinline__ void pw_layer_regs(f32x16 (&acc)[NB], __amdgpu_buffer_rsrc_t w_rsrc, unsigned w_lane,
                                              const f32x16 (&prev)[NP], float floor) {
  static_assert(NS == 4 * NP, "the previous layer's blocks are this layer's chunks");
  float4 wr[2][NB];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int n = 0; n < NB; ++n) wr[s][n] = pw_load4w(w_rsrc, w_lane, (unsigned)(n * NS + s) * 1024u);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float4 wc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) wc[n] = wr[s & 1][n];
    const int j = s >> 2, e = 4 * (s & 3);
    const float4 b = make_float4(fmaxf(prev[j][e], floor), fmaxf(prev[j][e + 1], floor), fmaxf(prev[j][e + 2], floor), fmaxf(prev[j][e + 3], floor));
    if (s + 2 < NS) {
#pragma unroll
      for (int n = 0; n < NB; ++n) wr[s & 1][n] = pw_load4w(w_rsrc, w_lane, (unsigned)(n * NS + s + 2) * 1024u);
    }
    __builtin_amdgcn_sched_barrier(0);
    PW_MFMA_STEP(acc, wc, b)
    __builtin_amdgcn_sched_barrier(0);
  }
}
#undef PW_MFMA_STEP

// (ReLU) + store of the last layer: NHWC 16-byte quads, or NCHW dwords (projection).  Pixels beyond M and channel quads beyond
// cout_store get an out-of-range offset and are dropped by the descriptor.
template <int NB, bool NCHW>
__device__ __forceinline__ void pw_store(const f32x16 (&acc)[NB], __amdgpu_buffer_rsrc_t o_rsrc, int m, bool m_ok, int hw,
                                         int cout_store, int ch0 /* first channel of acc[0] */, int fh, float floor) {
  const int img = NCHW ? m / hw : 0;
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = ch0 + 32 * n + 8 * g + 4 * fh;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = fmaxf(acc[n][4 * g + k], floor);
      if constexpr (!NCHW) {
        const unsigned off = (m_ok && ch < cout_store) ? (unsigned)(m * cout_store + ch) * 4u : PW_OOB;
        u32x4 pk;
        pk.x = __float_as_uint(v[0]); pk.y = __float_as_uint(v[1]); pk.z = __float_as_uint(v[2]); pk.w = __float_as_uint(v[3]);
        __builtin_amdgcn_raw_buffer_store_b128(pk, o_rsrc, off, 0, 0);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned off = (m_ok && ch + k < cout_store) ? (unsigned)((img * cout_store + ch + k) * hw + (m - img * hw)) * 4u : PW_OOB;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[k]), o_rsrc, off, 0, 0);
        }
      }
    }
}

}  // namespace

// KC: chunks of 32 in layer 0's K; NB0 / NB1 / NB2: 32-channel output blocks of the layers (0: no such layer); NPASS (single layer
// only): the layer has NPASS x NB0 blocks, computed NB0 at a time
template <int KC, int NB0, int NB1, int NB2, bool NCHW, int NPASS, int WAVES>
__global__ __launch_bounds__(256, WAVES) void conv_pw_kernel(PwLaunch p, int n_tiles) {
  static_assert(NB1 > 0 || NB2 == 0, "layers are consecutive");
  static_assert(NPASS == 1 || NB1 == 0, "passes over N: single layer only");
  constexpr int C0 = NPASS * NB0 * 32, C1 = NB1 * 32, C2 = NB2 * 32;
  __shared__ __attribute__((aligned(16))) float bias_s[C0 + C1 + C2];
  for (int i = threadIdx.x; i < C0; i += 256) bias_s[i] = p.layer[0].bias[i] + 0.0f;
  if constexpr (NB1 > 0)
    for (int i = threadIdx.x; i < C1; i += 256) bias_s[C0 + i] = p.layer[1].bias[i] + 0.0f;
  if constexpr (NB2 > 0)
    for (int i = threadIdx.x; i < C2; i += 256) bias_s[C0 + C1 + i] = p.layer[2].bias[i] + 0.0f;
  __syncthreads();          // the only one: from here on the waves run on their own

  const int lane = threadIdx.x & 63;
  const int fr = lane & 31, fh = lane >> 5;
  const int wave_g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int n_waves = (int)gridDim.x * 4;
  const int M = p.n_img * p.Ho * p.Wo;
  const int hw = p.Ho * p.Wo;
  const float ninf = -__builtin_huge_valf();
  const float floor0 = p.layer[0].relu ? 0.f : ninf;
  const float floor1 = p.layer[1].relu ? 0.f : ninf;
  const float floor2 = p.layer[2].relu ? 0.f : ninf;

  const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.in), 0, (int)((size_t)p.n_img * p.H * p.W * p.cin * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t o_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((size_t)M * p.cout_store * sizeof(float)), 0x00020000);
  constexpr int K0 = 32 * KC, K1 = 32 * NB0, K2 = 32 * NB1;
  const __amdgpu_buffer_rsrc_t w0_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.layer[0].w), 0, NPASS * NB0 * 32 * K0 * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t w1_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.layer[NB1 ? 1 : 0].w), 0, NB1 * 32 * K1 * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.layer[NB2 ? 2 : 0].w), 0, NB2 * 32 * K2 * 4, 0x00020000);
  const unsigned w_lane = (unsigned)lane * 16u;
  constexpr unsigned PASS_BYTES = (unsigned)(NB0 * 4 * KC) * 1024u;      // the fragments of one pass

  // the lane's byte offset of its pixel's first 16 bytes (tiles behind the last: out of range, the requests return zeros)
  auto pixel_offset = [&](int tile) -> unsigned {
    const int m = tile * 32 + fr;
    if (tile >= n_tiles || m >= M) return PW_OOB;
    int pix = m;
    if (p.stride != 1) {          // 1x1 / stride, no padding: output (oy, ox) reads input (stride oy, stride ox)
      const int img = m / hw, rem = m - img * hw;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      pix = (img * p.H + oy * p.stride) * p.W + ox * p.stride;
    }
    return (unsigned)(pix * p.cin + 4 * fh) * 4u;
  };

  int tile = wave_g, pass = 0;
  if (tile >= n_tiles) return;
  unsigned in_off = pixel_offset(tile);
  float4 bfirst[4], wfirst[2][NB0];
#pragma unroll
  for (int q = 0; q < 4; ++q) bfirst[q] = pw_load4(in_rsrc, in_off + 32 * q);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < NB0; ++n) wfirst[i][n] = pw_load4w(w0_rsrc, w_lane, (unsigned)(n * 4 * KC + i) * 1024u);

  // One unit of work; false behind the wave's last.  Forced inline: the first unit is peeled off the loop, so that the loop is only
  // ever entered with the request queue in its steady state (the counted waits at the loop's top are the minimum over its
  // entries: entered from the prologue's short queue they would wait for the previous unit's stores too).
  auto unit = [&]() __attribute__((always_inline)) -> bool {
    // the unit after this one: the tile's next pass, or the wave's next tile
    const int next_pass = pass + 1 < NPASS ? pass + 1 : 0;
    const int next_tile = next_pass ? tile : tile + n_waves;
    const unsigned in_off_next = next_pass ? in_off : pixel_offset(next_tile);
    const unsigned w_base = NPASS == 1 ? 0u : (unsigned)pass * PASS_BYTES;
    const unsigned w_base_next = NPASS == 1 ? 0u : (unsigned)next_pass * PASS_BYTES;
    const int m = tile * 32 + fr;
    const bool m_ok = m < M;

    f32x16 acc0[NB0];
    pw_init(acc0, bias_s + pass * NB0 * 32, fh);
    pw_layer_in<NB0, 4 * KC>(acc0, w0_rsrc, w_lane, w_base, w_base_next, in_rsrc, in_off, in_off_next, bfirst, wfirst);
    if constexpr (NB1 == 0) {
      pw_store<NB0, NCHW>(acc0, o_rsrc, m, m_ok, hw, p.cout_store, pass * NB0 * 32, fh, floor0);
    } else {
      f32x16 acc1[NB1];
      pw_init(acc1, bias_s + C0, fh);
      pw_layer_regs<NB1, 4 * NB0>(acc1, w1_rsrc, w_lane, acc0, floor0);
      if constexpr (NB2 == 0) {
        pw_store<NB1, NCHW>(acc1, o_rsrc, m, m_ok, hw, p.cout_store, 0, fh, floor1);
      } else {
        f32x16 acc2[NB2];
        pw_init(acc2, bias_s + C0 + C1, fh);
        pw_layer_regs<NB2, 4 * NB1>(acc2, w2_rsrc, w_lane, acc1, floor1);
        pw_store<NB2, NCHW>(acc2, o_rsrc, m, m_ok, hw, p.cout_store, 0, fh, floor2);
      }
    }
    if (next_tile >= n_tiles) return false;   // wave-uniform
    tile = next_tile; pass = next_pass; in_off = in_off_next;
    return true;
  };
  if (!unit()) return;
  while (unit()) {}
}

namespace {

template <int KC, int NB0, int NB1, int NB2, bool NCHW, int NPASS, int WAVES>
hipError_t pw_launch_cfg(const PwLaunch& c, hipStream_t s) {
  const int M = c.n_img * c.Ho * c.Wo;
  const int n_tiles = (M + 31) / 32;
  const int grid = persistent_grid(c.num_cu, (n_tiles + 3) / 4, WAVES);      // the workgroups that stay resident: WAVES waves per SIMD
  hipLaunchKernelGGL((conv_pw_kernel<KC, NB0, NB1, NB2, NCHW, NPASS, WAVES>), dim3(grid), dim3(256), 0, s, c, n_tiles);
  return hipGetLastError();
}

// the shape key of a launch: chunks of layer 0's K, then the 32-channel blocks of each layer
struct PwShape { int kc, nb[3]; bool ok; };
PwShape pw_shape(const PwLaunch& c) {
  PwShape r{0, {0, 0, 0}, false};
  if (c.n_layers < 1 || c.n_layers > 3 || !c.in || !c.out || c.num_cu <= 0) return r;
  if (c.cin % 4 != 0 || c.stride < 1 || c.n_img <= 0) return r;
  if (c.Ho != (c.H - 1) / c.stride + 1 || c.Wo != (c.W - 1) / c.stride + 1) return r;
  int k = c.layer[0].k_pad;
  if (k % 32 != 0 || k < c.cin) return r;
  r.kc = k / 32;
  for (int l = 0; l < c.n_layers; ++l) {
    const PwLayer& y = c.layer[l];
    if (!y.w || !y.bias || y.k_pad != k || y.cout_store % 4 != 0 || y.cout_store <= 0) return r;
    r.nb[l] = (y.cout_store + 31) / 32;
    if (r.nb[l] * 32 > y.cout_pad) return r;         // rows of the packed matrix / entries of the padded bias
    k = 32 * r.nb[l];                                // what the next layer's K must be: its input stays in registers
  }
  if (c.cout_store != c.layer[c.n_layers - 1].cout_store) return r;
  if (c.out_nchw && c.n_layers != 1) return r;
  // 32-bit byte offsets below PW_OOB
  if (!offsets_fit_32(c.n_img, c.H, c.W, c.cin) || !offsets_fit_32(c.n_img, c.Ho, c.Wo, c.cout_store)) return r;
  r.ok = true;
  return r;
}

}  // namespace

// (chunks of K, blocks of layer 0 per pass, blocks of layers 1 and 2, NCHW, passes, waves per SIMD).  The chains are bound by the
// matrix pipe and by their registers: two waves per SIMD.  Layer4's shortcut moves 0.23 GB for 0.05 ms of MFMAs: it is memory
// bound, so it takes two blocks at a time (four passes over pixels that stay in cache) in under 128 registers - four waves per
// SIMD, twice the requests in flight (141 us as two passes of four blocks at two waves, 117 us so; conv_igemm 122 us).
// Layer3's shortcut (64 -> 128 at 12x12, 0.45 GB) is NOT here: as X(2, 2, 0, 0, false, 2, 4) it took 161 us against conv_igemm's
// 157 us - both move its bytes at 2.8 - 2.9 TB/s, there is nothing left for a streaming kernel to remove - so it stays there.
#define UT_PW_SHAPES(X)                                                                              \
  X(5, 4, 3, 3, false, 1, 2) /* fusion 144 -> 108 -> 72 -> 72 */                                     \
  X(3, 3, 3, 3, false, 1, 2) /* temporal 90 (92) -> 90 x 3 */                                        \
  X(8, 3, 0, 0, true, 1, 2)  /* projection 256 -> 72, NCHW */                                        \
  X(4, 2, 0, 0, false, 4, 4) /* layer4 shortcut 128 -> 256 */
#define UT_PW_MATCH(KC, A, B, C, NCHW, NPASS) \
  (sh.kc == KC && sh.nb[0] == A * NPASS && sh.nb[1] == B && sh.nb[2] == C && (c.out_nchw != 0) == NCHW)

bool conv_pw_applicable(const PwLaunch& c) {
  const PwShape sh = pw_shape(c);
  if (!sh.ok) return false;
#define X(KC, A, B, C, NCHW, NPASS, WAVES) if (UT_PW_MATCH(KC, A, B, C, NCHW, NPASS)) return true;
  UT_PW_SHAPES(X)
#undef X
  return false;
}

hipError_t launch_conv_pw(const PwLaunch& c, hipStream_t s) {
  const PwShape sh = pw_shape(c);
  if (!sh.ok) return hipErrorInvalidValue;
#define X(KC, A, B, C, NCHW, NPASS, WAVES) if (UT_PW_MATCH(KC, A, B, C, NCHW, NPASS)) return pw_launch_cfg<KC, A, B, C, NCHW, NPASS, WAVES>(c, s);
  UT_PW_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

}  // namespace ut
