// Internal launch interface between the host orchestration (ut_api.hip; weights: ut_weights.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ut_split_pack.h"   // pack_split_weights, split_weight_scale

namespace ut {

// One convolution (1x1 or 3x3, stride 1 or 2) as an implicit GEMM over NHWC activations:
//   out[m][n] = act( sum_k A[m][k] * Wp[n][k] + bias[n] (+ res[m][n]) ),  m = (img, oy, ox)
// k is ordered (channel slice, tap, channel in slice) with slices of `cslice` channels:
//   k = s*(taps*cslice) + tap*cslice + c ,  input channel = s*cslice + c
// cslice = 32 when cin % 32 == 0 (one K chunk = one tap of one 128-byte channel slice, so the 9 taps
// of a slice re-read the same cache lines back to back and hit L1), else cslice = cin (tap major).
// Wp is [cout_pad][k_pad] k-contiguous, zero padded, BatchNorm folded.
struct ConvLaunch {
  const float* in;     // [n_img, H, W, cin]          (cin % 4 == 0)
  const float* w;      // [cout_pad][k_pad]
  const void* w_split; // optional: the two fp16 planes of (w * scale) in fragment order (conv_split.hip), or null
  float split_unscale; // 1 / scale of w_split
  int* status;         // split kernels: sticky status word, UT_SPLIT_RANGE is set when the input holds an infinity or a NaN
  const unsigned* in_max;   // split kernels: device word with the bits of the magnitude the activation scale is taken from (see
                            // split_act_scale): the handle's calibrated word of this tensor, or the word the producing kernel
                            // left in this call (publish_abs_max)
  const unsigned* in_obs;   // optional, with a calibrated in_max: the word the producer left in THIS call - an input beyond the
                            // calibrated range sets UT_SPLIT_RANGE
  int split_adaptive;       // with in_obs (UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE): an input outside the calibrated band takes its
                            // scale from in_obs instead (see split_act_scale) and counts one in *adapt_count
  unsigned* adapt_count;    // device word of the handle: launches that adapted (never null when split_adaptive is set)
  unsigned* out_max;        // optional device word (zero before the launch): receives the bits of max |out|
  const float* bias;   // [cout_pad]
  const float* res;    // optional residual, same layout as out
  float* out;          // NHWC [n_img, Ho, Wo, cout_store] or NCHW [n_img, cout_store, Ho*Wo]
  int n_img, H, W, cin, Ho, Wo;
  int cout_store;      // channels written per pixel (== channel stride of out / res)
  int cout_pad;        // rows of Wp (multiple of 128)
  int k_total;         // taps * cin
  int k_cin;           // conv_w4.hip, stride 1: input channels that K walks, a multiple of 32 in [64, cin] (0: cin).  Channels k_cin ..
                       // cin - 1 of `in` and their weight columns hold zeros (the regressor's tensors, padded to the kernel's shape):
                       // their products are exact zeros.  Strides, descriptors and the weight planes keep the padded sizes
  int cslice;          // channel slice width of the k order (32 or cin)
  int k_pad;           // row stride of Wp (multiple of 32)
  int ksize, stride, pad;
  int relu;
  int out_nchw;
  int device;          // HIP device the launch goes to (the dynamic-LDS attribute is set once per device)
  int num_cu;          // compute units of the device (persistent grid sizing)
  unsigned* tile_counter;   // device word, zero before the launch: dynamic tile queue of the persistent grid
  int no_resident;     // split kernels, A/B tests: the NO_* bits of the handle's ut_set_resident_weights kind (kResidentKinds below);
                       // read by choose_conv alone - no kernel and no shape predicate looks at it
  int splits;          // > 1 (latency mode): K is cut in `splits` equal chunk ranges, out = [splits][M][cout_store] slabs;
                       // 1 = latency mode without a split (prefers small tiles); 0 = throughput dispatch
};

hipError_t launch_conv_igemm(const ConvLaunch& c, hipStream_t s);
// latency mode: out = act(bias + res + sum of the split-K slabs, in slab order)
hipError_t launch_splitk_finish(const float* slabs, int n_splits, int m, int cout_store, const float* bias,
                                const float* res, float* out, int relu, hipStream_t s);
// One to three chained 1x1 convolutions (the first may have a stride; no padding) on the fp32 matrix instruction, a wave per 32
// output pixels, the intermediates of a chain in registers (conv_pw.hip): out = act_n(W_n ... act_0(W_0 in + b_0) ... + b_n),
// the bits of the same layers as consecutive conv_igemm launches.  Layer l + 1's k_pad must be 32 * ceil(cout_store_l / 32).
struct PwLayer {
  const float* w;      // ConvLaunch::w in fragment order: [cout_pad / 32][k_pad / 8][64 lanes][4], lane (fr = lane & 31, fh = lane >> 5)
                       // holding row 32 n + fr at k = 8 s + 4 fh .. + 3 (ut_weights.h::PackedConv::wfrag)
  const float* bias;   // [cout_pad]
  int k_pad, cout_store, cout_pad;
  int relu;
};
struct PwLaunch {
  const float* in;     // [n_img, H, W, cin]
  float* out;          // last layer: NHWC [n_img, Ho, Wo, cout_store] or NCHW [n_img, cout_store, Ho*Wo] (single layer only)
  PwLayer layer[3];
  int n_layers;
  int n_img, H, W, cin, Ho, Wo, stride;
  int cout_store;      // of the last layer
  int out_nchw;
  int num_cu;          // compute units of the device (grid sizing)
};
bool conv_pw_applicable(const PwLaunch& c);      // one of the shapes conv_pw.hip instantiates
hipError_t launch_conv_pw(const PwLaunch& c, hipStream_t s);
// the same convolution on the fp16 matrix cores from two-piece splits of both operands (conv_split.hip)
bool conv_split_applicable(const ConvLaunch& c);
hipError_t launch_conv_split(const ConvLaunch& c, hipStream_t s);
// the stride-2 entry of layer2: BasicBlock's first convolution (3x3 / 2, 32 -> 64, BN, ReLU) and its shortcut (1x1 / 2, 32 -> 64, BN)
// from one pass over the input (conv_c32s2.hip; split-fp16 arithmetic, weights resident in registers)
struct Stride2Launch {
  const float* in;          // [n_img][H][W][32]
  float* out1;              // [n_img][H/2][W/2][64]: relu(bn1(conv1 x))
  float* out2;              // [n_img][H/2][W/2][64]: bn_d(downsample x)
  const void* w1_split;     // pack_split_weights planes of the 3x3 ([cout_pad / 32][9][...]) and of the 1x1 ([cout_pad / 32][1][...])
  const void* wd_split;
  float unscale1, unscale_d;      // 1 / (their weight scales)
  const float* bias1;
  const float* bias_d;
  const unsigned* in_max;   // scale word of `in` (see ConvLaunch::in_max / in_obs / split_adaptive / adapt_count)
  const unsigned* in_obs;
  int split_adaptive;
  unsigned* adapt_count;
  unsigned* out1_max;       // device word (zero before the launch): receives the bits of max |out1|
  int* status;
  int n_img, H, W;
  int device, num_cu;
};
bool conv_c32s2_applicable(const Stride2Launch& c);
hipError_t launch_conv_c32s2(const Stride2Launch& c, hipStream_t s);
// 3x3 stride-1 from >= 64 channels to a multiple of 128 channels: four waves of 128 x 64, weights straight from global memory into
// registers, the patch split on its way into LDS, one barrier per slice (conv_w4.hip); conv_split_kernel<256, 128, 4, 2, true>'s bits
// the form a launch takes there: 128-channel tiles of the 12x12 / 6x6 maps, one 24x24 map x 64 channels, the phase planes of a stride-2 entry
enum W4Form : int { W4_NONE = 0, W4_TILES128, W4_MAP24, W4_STRIDE2 };
W4Form conv_w4_form(const ConvLaunch& c);
hipError_t launch_conv_w4(const ConvLaunch& c, hipStream_t s);
// Consecutive convolutions of conv_w4's stride-1 forms, each reading what the one before wrote, as ONE launch: a tile there is whole
// maps, so a workgroup takes its tiles depth-first through all layers (conv_w4.hip, CHAIN).  Per layer the bits of launch_conv_w4.
// The launches share shape, status word and device; the first one's tile_counter is the chain's, every layer keeps its own out_max
// word, and layer l + 1 is guarded against layer l's values as its own launch would be against layer l's word.
constexpr int W4_MAX_CHAIN = 9;
struct W4Layer {
  const float* in; const float* res; float* out; const void* w_split; const float* bias;
  const unsigned* in_max;   // the calibrated scale word of `in`
  unsigned* out_max;
  float split_unscale;
  int k_cin, relu;
};
struct W4ChainLaunch : ConvLaunch {      // the first layer's launch (shape, queue word, status, its guard), then every layer's record
  int n_layers;
  W4Layer lay[W4_MAX_CHAIN];
};
bool conv_w4_chainable(const ConvLaunch& a, const ConvLaunch& b);      // b may follow a in a chain
bool conv_w4_chain_fills(const ConvLaunch& c);      // a chain of launches like c keeps as many CUs busy as the launches themselves
hipError_t launch_conv_w4_chain(const ConvLaunch* layers, int n_layers, hipStream_t s);
// 3x3 stride-1 64 -> 64 channels with the weights resident in registers, K split across the two waves of a SIMD (conv_c64k.hip)
bool conv_c64k_applicable(const ConvLaunch& c);
hipError_t launch_conv_c64k(const ConvLaunch& c, hipStream_t s);
// One 32 -> 32 -> 32 channel BasicBlock (stride 1, no shortcut convolution) in one launch, split-fp16 arithmetic
// (conv_block32.hip): out = relu(conv2(relu(conv1(in) + bias1)) + bias2 + in), BatchNorm folded into weights and biases.
struct BlockLaunch {
  const float* in;          // [n_img, H, W, 32]
  float* out;               // [n_img, H, W, 32]
  const void* w1_split;     // ConvW::w_split of the two convolutions (fp16 planes in fragment order, pre-scaled)
  const void* w2_split;
  float unscale_w1, unscale_w2;   // 1 / weight scale
  const float* bias1;
  const float* bias2;
  float wsum1;              // max over output channels of sum_k |w1| (folded): bounds the intermediate with max|in| and bmax1
  float bmax1;              // max |bias1|
  const unsigned* in_max;   // scale word of `in` (never null; see ConvLaunch::in_max / in_obs / split_adaptive / adapt_count)
  const unsigned* in_obs;
  int split_adaptive;
  unsigned* adapt_count;
  unsigned* out_max;        // optional: receives the bits of max |out|
  int* status;
  unsigned* tile_counter;
  int n_img, H, W, device, num_cu;
};
bool conv_block32_applicable(const BlockLaunch& b);
hipError_t launch_conv_block32(const BlockLaunch& b, hipStream_t s);

// n 32-bit words := 0, as a kernel.  NOT hipMemsetAsync: captured into a hipGraph, a memset node of 16 bytes or more fills with
// a stale pattern from the second replay on (ROCm 7.2; tools/diag/graph_memset.py) - a garbage tile-queue word then walks a
// persistent kernel through ~10^9 tickets, which is what hung the whole-path graph replay of round 2.
hipError_t launch_zero_words(void* p, size_t n_words, hipStream_t s);
// *dst = max(*dst, *src) on two max words (one thread): the activation of several passes read by one consumer
hipError_t launch_merge_max(unsigned* dst, const unsigned* src, hipStream_t s);
// calibration: every non-zero finite word (the bits of a positive float) times 2^add_exp, exponent clamped below infinity
hipError_t launch_raise_words(unsigned* words, int n, int add_exp, hipStream_t s);
// n fp32 crops [n,96,96] of grey levels k / 255: the built-in calibration set of the split-fp16 activation scales (noise at
// several contrasts, gradients, bright blobs on a dark ground; counter-based, the same on every device)
hipError_t launch_calibration_crops(float* crops, int n, hipStream_t s);
// 3x3 stride-1 32->32 channel convs with the halo patch resident in LDS (conv_patch.hip)
bool conv_patch_applicable(const ConvLaunch& c);
hipError_t launch_conv_patch(const ConvLaunch& c, hipStream_t s);

// Which kernel runs a ConvLaunch: each launcher above runs its own kernel or refuses, choose_conv decides which one it is.
enum ConvKernel : int { CONV_IGEMM = 0, CONV_PATCH, CONV_SPLIT, CONV_W4, CONV_C64K };
constexpr const char* kConvKernelName[5] = {"conv_igemm", "conv_patch", "conv_split", "conv_w4", "conv_c64k"};

// ConvLaunch::no_resident: what an A/B kind of ut_set_resident_weights keeps split-fp16 launches off
enum : int {
  NO_C64K = 1,         // conv_c64k.hip
  NO_W4 = 2,           // conv_w4.hip in any form (its 128-channel tiles on the 12x12 / 6x6 maps have no bit of their own)
  NO_W4_MAP24 = 4,     // conv_w4.hip on the 24x24x64 maps (conv_c64k / the chunked kernel take layer2)
  NO_W4_STRIDE2 = 8,   // conv_w4.hip's phase-plane form on the stride-2 entries of layer3 / layer4 (the chunked gather kernel takes them)
  NO_W4_CHAIN = 16,    // conv_w4.hip's chains: every convolution its own launch (read by the host's collector, not by choose_conv)
};
constexpr int kResidentKinds[8] = {
    NO_C64K | NO_W4 | NO_W4_MAP24 | NO_W4_STRIDE2,            // 0: the chunked kernels everywhere
    0,                                                        // 1 (default): conv_w4 wherever it applies
    NO_W4 | NO_W4_MAP24 | NO_W4_STRIDE2,                      // 2: conv_c64k on 24x24, chunked elsewhere
    NO_C64K | NO_W4_STRIDE2,                                  // 3: conv_w4 on the stride-1 convolutions of all three sizes
    NO_W4_MAP24 | NO_W4_STRIDE2,                              // 4: conv_w4 at 12x12 / 6x6, conv_c64k at 24x24
    NO_C64K | NO_W4_MAP24 | NO_W4_STRIDE2,                    // 5: conv_w4 at 12x12 / 6x6, chunked at 24x24
    NO_W4_STRIDE2,                                            // 6: as 1 with the stride-2 entries through the chunked gather kernel
    NO_W4_CHAIN,                                              // 7: as 1, one launch per convolution
};
// (kinds 1 .. 6 chain wherever they send consecutive convolutions to conv_w4's stride-1 forms)

// the patch kernel's row of the dispatch: layer1's shape, except that latency mode (splits == 1) keeps a launch of fewer 64x64
// tiles than CUs on conv_igemm's small tiles (layer1 of a few crops: 144 small tiles beat 24 large ones)
inline bool conv_prefers_patch(const ConvLaunch& c) {
  const long m = (long)c.n_img * c.Ho * c.Wo;
  const bool few_tiles = ((m + 63) / 64) * ((c.cout_store + 63) / 64) <= (long)c.num_cu;
  return conv_patch_applicable(c) && !(c.splits == 1 && few_tiles);
}

// The one place that orders the kernels: first match wins (DESIGN.md section 4 reads it out by layer and mode).
inline ConvKernel choose_conv(const ConvLaunch& c) {
  if (c.splits > 1) return CONV_IGEMM;      // split-K launch of latency mode
  if (c.w_split && conv_split_applicable(c)) {      // split-fp16: conv_w4 in a form the kind allows, else conv_c64k, else chunked
    const int off = c.no_resident;      // the NO_* bits of the handle's kind
    const W4Form form = conv_w4_form(c);
    const int form_bit = form == W4_MAP24 ? NO_W4_MAP24 : form == W4_STRIDE2 ? NO_W4_STRIDE2 : 0;
    if (form != W4_NONE && !(off & (NO_W4 | form_bit))) return CONV_W4;
    if (conv_c64k_applicable(c) && !(off & NO_C64K)) return CONV_C64K;
    return CONV_SPLIT;
  }
  return conv_prefers_patch(c) ? CONV_PATCH : CONV_IGEMM;
}

// one convolution on kernel k; launch_conv: on the kernel choose_conv names, *ran (optional) receives which
inline hipError_t launch_conv_on(ConvKernel k, const ConvLaunch& c, hipStream_t s) {
  switch (k) {
    case CONV_PATCH: return launch_conv_patch(c, s);
    case CONV_SPLIT: return launch_conv_split(c, s);
    case CONV_W4: return launch_conv_w4(c, s);
    case CONV_C64K: return launch_conv_c64k(c, s);
    default: return launch_conv_igemm(c, s);
  }
}
inline hipError_t launch_conv(const ConvLaunch& c, hipStream_t s, ConvKernel* ran = nullptr) {
  const ConvKernel k = choose_conv(c);
  if (ran) *ran = k;
  return launch_conv_on(k, c, s);
}

// stem: conv3x3(1->32,pad 1)+BN+ReLU+maxpool2 ; crops [n,96,96] -> NHWC [n,48,48,32]
// out_max: optional device word (zero before the launch) that receives the bits of the largest output
hipError_t launch_stem(const float* crops, const float* w /*[32][9]*/, const float* bias /*[32]*/,
                       float* out, int n, unsigned* out_max, hipStream_t s);
// the same on the resampler's u8 grey levels (value / 255 on load)
hipError_t launch_stem_u8(const uint8_t* crops, const float* w, const float* bias, float* out, int n, unsigned* out_max,
                          hipStream_t s);

struct HeadBuffers {
  // workspace, all NHWC over the 6x6 map: [S,36,C]
  float* cat144;    // [S,36,144] canonical-space features of both views
  float* f108;      // [S,36,108]
  float* f72a;      // [S,36,72]
  float* f72b;      // [S,36,72] fusion output (canonical space)
  float* fused;     // [S,36,72] cam0-space fused features (input of the temporal block)
  float* t92a;      // [S,36,92] temporal ping
  float* t92b;      // [S,36,92] temporal pong
  float* regin;     // [S,36,C] regressor input (C = 76 or 72; 128 with zero channels when its convolutions run in split-fp16)
  float* rega;      // [S,36,C]
  float* regb;      // [S,36,C]
  float* skel;      // [n_skel,36,4]
  float* xf;        // [S,40] per-sample transforms: A0(12) A1(12) s0(1) rel(12) flags
};

// Bits of the sticky device status word written by the index checks (ut_api.hip turns them into UT_E_INVALID).
enum : int {
  UT_BAD_SAMPLE_RANGE = 1,   // a sample_range row is not 1 or 2 crops inside [0, n_crops]
  UT_BAD_MEMORY_IDX = 2,     // memory_idx outside [0, n_slots)
  UT_DUP_MEMORY_IDX = 4,     // two samples of one call name the same temporal slot
  UT_BAD_HAND_IDX = 8,       // hand_idx not 0 / 1
  UT_SINGLE_VIEW = 16,       // informational: at least one one-view sample (an error only in unknown-skeleton mode)
  UT_BAD_SRC_INDEX = 32,     // ut_warp_crops: src_index outside [0, n_src_images)
  UT_SPLIT_RANGE = 64,       // split-fp16 convolutions: an input activation is an infinity or a NaN (nothing to scale by)
};
constexpr int UT_STATUS_ERRORS = UT_BAD_SAMPLE_RANGE | UT_BAD_MEMORY_IDX | UT_DUP_MEMORY_IDX | UT_BAD_HAND_IDX | UT_BAD_SRC_INDEX | UT_SPLIT_RANGE;

#if defined(__HIPCC__)
// ---- activation range of the split-fp16 arithmetic -------------------------------------------------------------------
// Every kernel whose output a split convolution reads leaves the bits of max |out| in a device word (the values are
// compared as unsigned integers: for non-negative floats that is the float order, an infinity or a NaN compares above
// every finite value).  The consumer turns the word into a power of two 2^k that puts the largest activation in
// [2^14, 2^15), multiplies every activation by it before the two-piece split (exact in fp32) and folds 2^-k into the
// epilogue's factor: the first piece then never saturates and the second stays a normal fp16 number for every activation
// within 2^-18 of the layer's largest - the split has fp32's exponent range instead of fp16's, with no precondition on
// the network's activation magnitudes (lib/models/backbone_resnet.py:56-72 has none either).
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// one relaxed look first: after the first few workgroups the word is near its final value and the atomic is skipped
__device__ __forceinline__ void publish_abs_max(unsigned* word, unsigned lane_bits) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)lane_bits, o);
    lane_bits = other > lane_bits ? other : lane_bits;
  }
  if ((threadIdx.x & 63) == 0 && lane_bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(word, lane_bits);
}

// scale = 2^k, unscale = 2^-k with k = 141 - e for a magnitude of biased exponent e - a value in [2^(e - 127), 2^(e - 126)) times 2^k is
// in [2^14, 2^15) - kept within +-100; k = 0 (scale 1) when the magnitude has `none` (zero, an infinity, a NaN).  Returns k.
__device__ __forceinline__ int split_pow2_for(int e, bool none, float& scale, float& unscale) {
  int k = none ? 0 : 141 - e;
  k = k > 100 ? 100 : k < -100 ? -100 : k;
  scale = __uint_as_float((unsigned)(127 + k) << 23);
  unscale = __uint_as_float((unsigned)(127 - k) << 23);
  return k;
}

// scale = 2^k, unscale = 2^-k; ok = false when the word holds an infinity / a NaN (scale 1 then).
// in_obs (optional): the largest magnitude the producer actually stored in this call, when in_max is a calibrated word: the
// first piece of x * 2^k stays finite while x * 2^k < 2^16, i.e. while x's exponent is at most one above the word's;
// beyond that (or a non-finite value) ok = false.
// adaptive (with in_obs; UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE): a finite non-zero in_obs outside the calibrated band - beyond
// that guard, or more than 11 binades below the word (under 2^-7 of the calibration maximum, the word being 2^4 x it) - is
// taken as the scale word instead, exactly as a dynamic-scale launch takes its producer's word: adapted = true, ok = true.
// A zero in_obs, an infinity or a NaN never adapts.  Every workgroup reads the same two words, so the choice is uniform over
// the launch.  Returns the bits the scale was taken from.
__device__ __forceinline__ unsigned split_act_scale(const unsigned* in_max, const unsigned* in_obs, bool adaptive, float& scale,
                                                    float& unscale, bool& ok, bool& adapted) {
  unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane((int)*in_max);
  const unsigned obs = in_obs ? (unsigned)__builtin_amdgcn_readfirstlane((int)*in_obs) : 0u;
  const int eo = (int)(obs >> 23);
  int e = (int)(bits >> 23);
  int k = split_pow2_for(e, bits == 0u || e == 255, scale, unscale);
  adapted = adaptive && in_obs && obs != 0u && eo != 255 && (eo + k > 142 || eo + 11 < e);
  if (adapted) {
    bits = obs;
    e = eo;
    k = split_pow2_for(e, false, scale, unscale);
  }
  ok = e != 255;
  if (in_obs && !adapted && (eo == 255 || eo + k > 142)) ok = false;      // 2^(eo - 127) * 2^k >= 2^16
  return bits;
}

// block 0's first thread reports the launch: UT_SPLIT_RANGE when !ok, one count in *adapt_count when it adapted
__device__ __forceinline__ void split_scale_report(bool ok, bool adapted, int* status, unsigned* adapt_count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (!ok && status) atomicOr(status, UT_SPLIT_RANGE);
    if (adapted && adapt_count) atomicAdd(adapt_count, 1u);
  }
}
#endif

struct HeadArgs {
  const float* feat;        // [N,72,36] NCHW
  const float* intrinsics;  // [N,3,3]
  const float* extrinsics;  // [N,4,4]
  const int64_t* sample_range;
  const int64_t* memory_idx;
  const uint8_t* use_memory;
  const int64_t* hand_idx;
  int n_samples;
  int n_crops;
  int n_slots;
  float* mem;               // [slots,36,18] NHWC temporal memory
  float* prev_ext;          // [slots,16]
  int* status;              // device words: [0] sticky error bits (UT_* above), [1] bits of THIS call (zero on entry).
                            // Kernels that index with the descriptors return when status[0] has an error bit or
                            // status[1] a bit of call_error_mask: nothing is read or written out of range and the
                            // temporal state stays as it was
  int call_error_mask;      // UT_SINGLE_VIEW in unknown-skeleton mode (lib/models/umetrack_model.py:224-229), else 0
  int* slot_seen;           // [n_slots] scratch of the duplicate check, zero on entry
};

// One pass over the frame descriptors before anything indexes with them (stream ordered).
hipError_t launch_validate_desc(const HeadArgs& a, hipStream_t s);

// staged: the sample's values leave through LDS with consecutive lanes on consecutive channels; else every lane stores its own
// pixel's values 576 (288) bytes apart.  Same expression per element: same bits.
hipError_t launch_ftl_in(const HeadArgs& a, const HeadBuffers& b, bool staged, hipStream_t s);
hipError_t launch_ftl_out_temporal_in(const HeadArgs& a, const HeadBuffers& b, hipStream_t s);
// regin [S,36,reg_stride]: channels reg_c .. reg_stride - 1 are zeroed; out_max (optional, zero before the launch): max |regin|
hipError_t launch_temporal_out(const HeadArgs& a, const float* t_out /*[S,36,92]*/, const float* skel,
                               int n_skel, float* regin, int reg_c, int reg_stride, unsigned* out_max, hipStream_t s);
hipError_t launch_skeleton(const float* skel_in /*[n_skel,2,22,3]*/, const float* w /*[144][132]*/,
                           const float* bias /*[144]*/, const float* bn_scale /*[4]*/,
                           const float* bn_shift /*[4]*/, float* out /*[n_skel,36,4]*/, int n_skel,
                           hipStream_t s);
// avgpool(6x6) -> 1x1 conv (C->D) -> decode -> world transform -> pose record [S,60]
hipError_t launch_pool_decode(const HeadArgs& a, const float* reg_feat /*[S,36,reg_stride]*/, int reg_c, int reg_stride,
                              const float* w /*[D][C]*/, const float* bias /*[D]*/, int d,
                              float* out_pose, float* out_raw, float* raw_ws /*[S,64] scratch*/, hipStream_t s);

hipError_t launch_fk(const float* hand_model, int n_models, const float* ja, int ja_stride,
                     const float* xf, int xf_stride, const int64_t* mirror, float t_scale, int n,
                     float* out, hipStream_t s);

// Poses from landmarks, the inverse of launch_fk: one Levenberg-Marquardt solver (ut_fit_dev.h), one wave per pose, under four
// costs.  FitPoseArgs is what the four entries share; pointers as ut_fit_pose documents them.
struct FitPoseArgs {
  const float* hand_model; int n_models;
  const float* targets; int target_stride;
  const float* limits;                  // [n_models,20,2] or null
  const float* init_ja; int init_ja_stride;
  const float* init_xf; int init_xf_stride;   // both init pointers null: cold start
  const int64_t* mirror;
  float t_scale;
  int max_iters, n;
  float* ja; int ja_stride;
  float* xf; int xf_stride;
};
enum : int { FIT_CONVERGED = 1, FIT_AT_MAX_ITERS = 2, FIT_REFUSED = 4 };      // UT_FIT_*, and the low bits of UT_FITS_*

// fit.hip: scalar weights, the cost sum_l w_l |landmark_l - target_l|^2.
struct FitArgs {
  FitPoseArgs pose;
  const float* weights;                 // [n,21] or null
  float* info;                          // [n,4] or null
};
hipError_t launch_fit_pose(const FitArgs& a, hipStream_t s);

// fit_info.hip: landmarks with their information, the residuals whitened by a 3 x 3 factor per landmark.  Pointers as
// ut_fit_pose_info documents them.
struct FitInfoArgs {
  FitPoseArgs pose;
  const float* sqrt_info;               // [n,21,6]: l00 l10 l11 l20 l21 l22 of the lower factor of a landmark's information
  float* info;                          // [n,4] or null
};
hipError_t launch_fit_pose_info(const FitInfoArgs& a, hipStream_t s);

// fit_views.hip: no 3-D targets (pose.targets is null), the cost is the reprojection error of the landmarks in camera views.
// Pointers as ut_fit_pose_views documents them; kind is PROJECT_FISHEYE62 or PROJECT_PINHOLE, max_views 1..TRI_MAX_VIEWS (below).
struct FitViewsArgs {
  FitPoseArgs pose;
  const double* window;                 // [n,max_views,21,2]
  const float* weights;                 // [n,max_views,21] or null
  const int32_t* cam_rows;              // [n,max_views] row of `table`, -1 = unused view
  int max_views;
  const double* table;                  // [n_rows,32] or [n_rows,24]
  int n_rows, kind;
  float* info;                          // [n,4] or null
  float* residual;                      // [n,max_views,21] or null
  int* status;                          // sticky status word: UT_BAD_SRC_INDEX for a cam_rows entry outside [-1, n_rows)
};
hipError_t launch_fit_pose_views(const FitViewsArgs& a, hipStream_t s);

// fit_views_robust.hip: the same fit under a robust loss (ut_fit_pose_views_robust).  FitViewsArgs itself is a kernel argument of
// fit_views.hip, whose device code stays what it is, so the loss's three fields stand behind it here and not inside it.
enum : int { FITV_LOSS_SQUARED = 0, FITV_LOSS_HUBER = 1, FITV_LOSS_GEMAN_MCCLURE = 2 };
struct FitViewsRobustArgs {
  FitViewsArgs views;
  int loss;                             // FITV_LOSS_*
  float loss_scale;                     // px, finite and > 0; not read by FITV_LOSS_SQUARED
  float* inlier;                        // [n,max_views,21] or null: psi of every used observation at the returned pose, 0 elsewhere
};
hipError_t launch_fit_pose_views_robust(const FitViewsRobustArgs& a, hipStream_t s);

// fit_scale.hip: fit.hip's cost with ln(scale) of the hand as a 27th parameter, and the pool of per-pose scales, one wave per
// group.  Pointers as ut_fit_pose_scale / ut_pool_scale document them; the constants are public as UT_SCALE_* / UT_FITS_*.
constexpr int FITS_MODE_FREE = 0, FITS_MODE_FIXED = 1;
constexpr float FITS_SCALE_MIN = 0.25f, FITS_SCALE_MAX = 4.0f, FITS_SCALE_INFO_LAMBDA = 1e-6f;
enum : int { FITS_CONVERGED = FIT_CONVERGED, FITS_AT_MAX_ITERS = FIT_AT_MAX_ITERS, FITS_REFUSED = FIT_REFUSED, FITS_AT_BOUND = 8 };
struct FitScaleArgs {
  FitPoseArgs pose;
  const float* weights;                 // [n,21] or null
  const float* init_scale;              // [n] or null = 1
  int scale_mode;
  float* scale;                         // [n]
  float* info;                          // [n,6] or null
};
hipError_t launch_fit_pose_scale(const FitScaleArgs& a, hipStream_t s);
hipError_t launch_pool_scale(const float* scale, const float* info, int n_groups, int group_size, float* group,
                             float* pose_scale, hipStream_t s);

// fit_views_scale.hip: the fit in the views, every loss, with ln(scale) as a 27th parameter (ut_fit_pose_views_scale).  The scale's
// fields stand behind FitViewsRobustArgs as the loss's stand behind FitViewsArgs; robust.views.info is [n,6] here, the row layout
// launch_pool_scale reads.
struct FitViewsScaleArgs {
  FitViewsRobustArgs robust;
  const float* init_scale;              // [n] or null = 1
  int scale_mode;                       // FITS_MODE_*
  float* scale;                         // [n]
};
hipError_t launch_fit_pose_views_scale(const FitViewsScaleArgs& a, hipStream_t s);

// pose_info_views.hip: the information of a pose under the cost of the fits in the views (ut_pose_information_views).  The pose
// stands where the fit has its start (robust.views.pose.init_ja / init_xf); the pose outputs, limits, max_iters, views.info and
// views.residual are not read.  Pointers as ut_pose_information_views documents them; the constants are public as UT_COV_*.
enum : int { COV_OK = 1, COV_SINGULAR = 2, COV_REFUSED = FIT_REFUSED };
constexpr float COV_MIN_PIVOT = 0x1p-16f;
struct PoseInfoViewsArgs {
  FitViewsRobustArgs robust;
  const float* angle_sigma;             // [n_models,20] or null
  float* pose_info;                     // [n,351] or null
  float* pivot;                         // [n,3] or null
  float* param_sigma;                   // [n,26] or null
  float* landmark_cov;                  // [n,21,6] or null
  float* info;                          // [n,4] or null
};
hipError_t launch_pose_information_views(const PoseInfoViewsArgs& a, hipStream_t s);

// smooth.hip: fitted poses smoothed over a sequence by their information matrices (ut_smooth_pose_sequence).  Pointers as
// ut_smooth_pose_sequence documents them; the constants are public as UT_SMOOTH_*.
enum : int { SMOOTH_OK = 1, SMOOTH_SINGULAR = 2, SMOOTH_REFUSED = FIT_REFUSED, SMOOTH_GAP = 8 };
constexpr int SMOOTH_WORK = 408;
struct SmoothArgs {
  const float* ja; int ja_stride;
  const float* xf; int xf_stride;
  const float* pose_info;               // [n_seq * n_frames,351]
  const float* pivot;                   // [n_seq * n_frames,3]
  const float* frame_weight;            // [n_seq * n_frames] or null
  const int32_t* lengths;               // [n_seq] or null
  const float* centre;                  // [n_seq,3] or null
  const float* step_var; int n_var;     // [n_var,26]
  float t_scale;
  int n_seq, n_frames;
  float* workspace;                     // [n_seq * n_frames,SMOOTH_WORK]
  float* ja_out; int ja_out_stride;
  float* xf_out; int xf_out_stride;
  float* param_sigma;                   // [n_seq * n_frames,26] or null
  float* info;                          // [n_seq * n_frames,4] or null
};
hipError_t launch_smooth_pose_sequence(const SmoothArgs& a, hipStream_t s);

// start_views.hip: starts for the fits in the views from the detections alone (ut_start_pose_views), and the selection among fitted
// candidates (ut_select_pose).  Of views.pose the model, limits, mirror, t_scale, n and the outputs (n * n_bank rows) are read;
// views.info is [n * n_bank,4]; views.residual is not read.  Pointers as umetrack_hip_start.h documents them.
struct StartViewsArgs {
  FitViewsArgs views;
  const float* bank; int n_bank;        // [n_bank,20]
  const double* seeds; int n_seeds;     // [n_seeds,9]
  int iters;
};
hipError_t launch_start_pose_views(const StartViewsArgs& a, hipStream_t s);
struct SelectPoseArgs {
  const float* ja; int ja_stride;
  const float* xf; int xf_stride;
  const float* info;                    // [n * n_cand,4]
  int n, n_cand;
  float* out_ja; int out_ja_stride;
  float* out_xf; int out_xf_stride;
  float* out_info;                      // [n,4] or null
  int32_t* out_index;                   // [n] or null
};
hipError_t launch_select_pose(const SelectPoseArgs& a, hipStream_t s);

// track_views.hip: sequences of detections followed frame by frame in one launch (ut_track_pose_views), one wave per sequence.  The
// tracker's fields stand behind FitViewsRobustArgs as the loss's stand behind FitViewsArgs.  robust.views.pose: n = n_seq * n_frames,
// init_ja / init_xf the sequences' starts [n_seq] or null; robust.views.info is required; residual and inlier are not written.
// Pointers as umetrack_hip_track.h documents them; the constants are public as UT_TRACK_*.
enum : int { TRACK_WARM = 0, TRACK_COLD = 1, TRACK_NONE = 2 };
struct TrackViewsArgs {
  FitViewsRobustArgs robust;
  const float* cold_ja; int cold_ja_stride;   // [n_seq * n_frames] rows, or all four cold pointers null: no recovery
  const float* cold_xf; int cold_xf_stride;
  const float* cold_info;               // [n_seq * n_frames,4]
  const int32_t* cold_index;            // [n_seq * n_frames], < 0: the cold row is refused
  double recover_ratio, recover_floor;
  const int32_t* lengths;               // [n_seq] or null
  int n_seq, n_frames;
  int32_t* chosen;                      // [n_seq * n_frames]
};
hipError_t launch_track_pose_views(const TrackViewsArgs& a, hipStream_t s);

// Linear blend skinning of a packed mesh (mesh.hip), one workgroup per pose; pose arguments as for launch_fk.
//  verts    float4 [nv][2]: (x, y, z, bits: bone index of slot k in byte k) | the four slot weights, slots sorted by ascending
//           bone, unused slots weight 0 / bone 0
//  csr_off  [nv + 1], csr_ent [3 * n_triangles]: per vertex its incident triangles in ascending triangle order, each entry the
//           triangle's other two vertices in winding order, first | second << 16
//  out_v [n,nv,3]; out_n [n,nv,3] or null (no normals).
// The posed vertices of a pose stay in LDS until its normals are done: 12 nv bytes of dynamic LDS next to 4848 static ones.
// MESH_MAX_VERTICES is what fits the 64 KB a workgroup gets without a per-device function attribute (65536 - 4848 = 60688
// >= 12 * 5056); it also keeps a vertex index in 16 bits (csr_ent).  Public as UT_MESH_MAX_VERTICES.
constexpr int MESH_MAX_VERTICES = 5056;
hipError_t launch_skin_mesh(const float* hand_model, int n_models, const float* ja, int ja_stride, const float* xf,
                            int xf_stride, const int64_t* mirror, float t_scale, int n, const void* verts,
                            const uint32_t* csr_off, const uint32_t* csr_ent, int nv, float* out_v, float* out_n,
                            hipStream_t s);

// World points into camera windows (render.hip), one thread per (pose, view, point).
enum : int { PROJECT_FISHEYE62 = 0, PROJECT_PINHOLE = 1 };
struct ProjectArgs {
  const float* points;          // [n] rows of point_stride floats, the first 3 * n_points of a row are its points
  int point_stride, n_points;
  const int32_t* cam_rows;      // [n,max_views] row of `table`, -1 = unused view
  int max_views;
  const double* table;          // [n_rows,32] source cameras (PROJECT_FISHEYE62) or [n_rows,24] crop cameras (PROJECT_PINHOLE)
  int n_rows, kind, n;
  int width, height;            // bit 1 of flags: inside [0,width) x [0,height)
  double* window;               // [n,max_views,n_points,2]
  double* eye_z;                // [n,max_views,n_points]
  uint8_t* flags;               // [n,max_views,n_points]
  int* status;                  // sticky status word: UT_BAD_SRC_INDEX for a cam_rows entry outside [-1, n_rows)
};
hipError_t launch_project_points(const ProjectArgs& g, hipStream_t s);

// Window points back into the world (triangulate.hip), the inverse of launch_project_points: one thread per (pose, point).
// Pointers as ut_triangulate_points documents them; kind is PROJECT_FISHEYE62 or PROJECT_PINHOLE.
constexpr int TRI_MAX_VIEWS = 8;
enum : int { TRI_CONVERGED = 1, TRI_AT_MAX_ITERS = 2, TRI_REFUSED = 4, TRI_DEGENERATE = 8 };
struct TriArgs {
  const double* window;         // [n,max_views,n_points,2]
  const float* weights;         // [n,max_views,n_points] or null
  const int32_t* cam_rows;      // [n,max_views] row of `table`, -1 = unused view
  int max_views;
  const double* table;          // [n_rows,32] or [n_rows,24]
  int n_rows, kind, n_points, n, max_iters;
  double* points;               // [n,n_points,3] or null
  float* points_f32;            // [n] rows of point_stride floats, or null
  int point_stride;
  float* info;                  // [n,n_points,4] or null
  float* residual;              // [n,max_views,n_points] or null
  int* status;                  // sticky status word: UT_BAD_SRC_INDEX for a cam_rows entry outside [-1, n_rows)
  float* sqrt_info;             // [n,n_points,6] or null: l00 l10 l11 l20 l21 l22 of the lower Cholesky factor of H at the point
};
hipError_t launch_triangulate(const TriArgs& a, hipStream_t s);

// Posed meshes rasterised into 96x96 crop cameras (render.hip), one workgroup per (pose, view).
//  tris int4 [nt]: (a, b, c, 0) per triangle.  The projected vertices of a pose (12 nv bytes, dynamic) share the workgroup's LDS
//  with a 48 x 96 plane of 64-bit (depth, triangle) words (36864 bytes): RENDER_MAX_VERTICES is what fits the 64 KB a workgroup
//  gets without a per-device function attribute (65536 - 36864 = 28672 >= 12 * 2368).  Public as UT_RENDER_MAX_VERTICES.
constexpr int RENDER_CROP = 96;
constexpr int RENDER_MAX_VERTICES = 2368;
struct RenderArgs {
  const float* vertices;        // [n,nv,3] world
  int nv;
  const int4* tris;
  int nt;
  const double* crop_params;    // [n_crops,24]
  const int64_t* sample_range;  // [n,2]
  int n, n_crops;
  float* depth;                 // [n_crops,96,96] or null
  int32_t* tri;                 // [n_crops,96,96] or null
  uint8_t* shade;               // [n_crops,96,96] or null
  int* status;                  // sticky status word: UT_BAD_SAMPLE_RANGE
};
hipError_t launch_render_check(const RenderArgs& g, hipStream_t s);
hipError_t launch_render_mesh(const RenderArgs& g, hipStream_t s);

// Batched crop-camera generation (cropgen.hip): one candidate = one (frame, hand) label pose.
struct CropGenArgs {
  const double* cam_params;     // [n_frames*n_cams,32] source camera rows (layout of ut_warp_crops)
  const double* camera_angles;  // [n_cams] degrees
  const float* hand_model;      // [n_models,321]
  const float* joint_limits;    // [n_models,22,2]
  const float* joint_angles;    // [n,22]
  const float* wrist_xf;        // [n,4,4] (mm)
  const int32_t* frame_idx;     // [n]
  const int64_t* hand_idx;      // [n]
  int n, n_models, n_cams, max_views, min_vis, src_w, src_h, crop_size;
  double focal_multiplier;
  double* crop_params;          // [n,max_views,24]
  float* intrinsics;            // [n,max_views,3,3]
  float* extrinsics;            // [n,max_views,4,4]
  int32_t* cam_index;           // [n,max_views]  (-1 = unused slot)
  int32_t* n_views;             // [n]
  int32_t* status;              // [n] 0 ok, 1 = "Unable to create crop camera"
  float* landmarks;             // optional [n,21,3]: world landmarks of the label pose (mm)
};
hipError_t launch_cropgen(const CropGenArgs& g, hipStream_t s);

// label-free crop cameras from 21 window keypoints per (hand, view) (lib/tracker/tracker.py:111-219)
struct CropGenWindowArgs {
  const double* cam_params;     // [n_cam_rows,32] Fisheye62 source camera rows (layout of ut_warp_crops)
  const double* keypoints;      // [n,max_views,21,2] window px
  const int32_t* src_row;       // [n,max_views] row of cam_params, -1 = not seen in that view (checked by the caller)
  const int64_t* hand_idx;      // [n] 0 / 1 (1 = x-mirrored crop)
  int n, max_views, crop_size;
  double focal_multiplier;
  double* crop_params;          // [n,max_views,24]
  float* intrinsics;            // [n,max_views,3,3]
  float* extrinsics;            // [n,max_views,4,4]
  int32_t* cam_index;           // [n,max_views] src_row of the view in that slot (-1 = unused slot)
  int32_t* n_views;             // [n]
  int32_t* status;              // [n] 0 ok, 1 = "Unable to create crop camera"
};
hipError_t launch_cropgen_window(const CropGenWindowArgs& g, hipStream_t s);

// torch_data path: crop matrices per (frame, view) and the pinhole->pinhole homography resampler.
struct CropMatArgs {
  const float* orig_extrinsics;  // [n_frames*n_views,4,4] world->eye
  const float* orig_intrinsics;  // [n_frames*n_views,3,3]
  const float* crop_points;      // [n_frames,n_pts,3]
  const int64_t* hand_idx;       // [n_frames] (1 = right hand = mirrored crop)
  int n_frames, n_views, n_pts, crop_size;
  double focal_multiplier;
  float* extrinsics_xf;          // [n_frames*n_views,4,4]
  float* new_intrinsics;         // [n_frames*n_views,3,3]
  float* resample_xf;            // [n_frames*n_views,4,4]
  int32_t* status;               // [n_frames*n_views]
};
hipError_t launch_cropmat(const CropMatArgs& g, hipStream_t s);
hipError_t launch_resample_homography(const void* src, int src_is_f32, int n, int src_h, int src_w,
                                      const float* resample_xf, int out_h, int out_w, float* out, hipStream_t s);

hipError_t launch_keypoint_metrics(const float* gt, const float* tracked, const uint8_t* valid, int n_hands, int n_frames,
                                   double* err, double* acc, double* gt_acc, uint8_t* valid_acc, hipStream_t s);

hipError_t launch_mem_export(const float* mem /*[slots,36,18]*/, float* out /*[slots,18,36]*/, int slots, hipStream_t s);

// status: device word; a crop whose src_index is outside [0, n_src) is written as zeros and sets UT_BAD_SRC_INDEX.
// out_u8 != NULL (mode 0 only): write the grey levels as u8 instead of out = level / 255.
hipError_t launch_warp(const uint8_t* src, int n_src, int src_h, int src_w, const double* cam,
                       const double* crop, const int32_t* src_index, int n_crops, int mode, float* out,
                       uint8_t* out_u8, int* status, hipStream_t s);

// diagnostic: the fp32 coordinate map of every crop, [n_crops, 96, 96, 2] (x, y); a bad src_index gives (-1, -1)
hipError_t launch_warp_map(const double* cam, const double* crop, const int32_t* src_index, int n_src, int n_crops,
                           float* out, hipStream_t s);

}  // namespace ut
