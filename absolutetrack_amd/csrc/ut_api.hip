// C ABI of libumetrack_hip.so (include/umetrack_hip.h): handle, weight upload, workspace, temporal state
// and the launch sequences of the hot path.  Host-only logic; kernels live in the other translation
// units, weight folding and packing in ut_weights.cpp.
#include "../../include/umetrack_hip.h"
#include "../../include/umetrack_hip_fit.h"
#include "../../include/umetrack_hip_info.h"
#include "../../include/umetrack_hip_robust.h"
#include "../../include/umetrack_hip_scale.h"
#include "../../include/umetrack_hip_smooth.h"
#include "../../include/umetrack_hip_start.h"
#include "../../include/umetrack_hip_track.h"
#include "../../include/umetrack_hip_triangulate.h"
#include "../../include/umetrack_hip_uncertainty.h"
#include "../../include/umetrack_hip_views.h"
#include "../../include/umetrack_hip_views_scale.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ut_kernels.h"
#include "ut_weights.h"

namespace {

thread_local std::string g_create_error;

struct ConvW : ut::ConvGeom {
  float* w = nullptr;     // device [cout_pad][k_pad]
  float* w_frag = nullptr;   // device, only the 1x1 convolutions conv_pw.hip takes: the same matrix in its fragment order (PackedConv::wfrag)
  void* w_split = nullptr;   // device: the two fp16 planes of w * 2^k in fragment order (conv_split.hip), eligible layers only
  float split_unscale = 0.f; // 2^-k
  float wsum_rows = 0.f;     // max over output channels of sum_k |w| (folded), rounded up: bounds |conv(x)| by wsum_rows * max|x|
  float bias_max = 0.f;      // max |bias| (folded)
  float* bias = nullptr;  // device [cout_pad]
  int k_cin = 0;          // > 0: input channels behind k_cin are zero padding in activations and weights (ConvLaunch::k_cin)
};

struct Block {
  ConvW conv1, conv2, ds;
  bool has_ds = false;
};

struct Regressor {
  Block blocks[2];
  Block blocks_split[2];    // the same convolutions with input and output channels zero-padded to 128: the shape conv_w4.hip takes
  float* w_out = nullptr;   // [D][C] raw (applied after the average pool)
  float* b_out = nullptr;
  int c = 0, d = 0;
};

struct ProfEvent { hipEvent_t a, b; double flops;   int kind = 0;   // 0: fp32 matrix-instruction kernels, 1: split-fp16 kernels
  int convs = 1;      // convolutions the bracket counts for: the layers of a conv_w4 chain (one launch, one pair of events)
};

}  // namespace

constexpr int kDefaultChunk = 4096;
constexpr int kMaxChunk = 7281;   // 48*48*32*4 B per crop under 2^31 - 256 bytes

struct ut_context {
  int device = 0;
  int num_cu = 256;
  std::string err;
  std::vector<void*> allocs;        // everything to hipFree at destroy
  // weights
  float* stem_w = nullptr; float* stem_b = nullptr;
  Block bb[12];
  ConvW proj, fus0, fus1, fus2, tmp[3];
  float *skel_w = nullptr, *skel_b = nullptr, *skel_scale = nullptr, *skel_shift = nullptr;
  Regressor reg_k, reg_u;
  // backbone workspace.  Phase A (stem, layer1, layer2) runs in passes of `chunk` crops: bounded by the 32-bit
  // byte offsets of the buffer descriptors (a 48x48x32 fp32 map is 295 KB per crop -> at most 7281 crops) and
  // by memory (4.2 GB of workspace at 4096); the convolutions are matrix-pipe bound, so fewer, larger launches
  // win over cache residency (measured: 1024 -> 4096 crops per pass = +1.6 % end to end).  Phase B (layer3,
  // layer4, projection) runs over up to PHASE_B_MAX crops at once so that the small late maps still fill the
  // chip with workgroups.
  int chunk = kDefaultChunk;
  size_t ws_crops = 0;    // phase-A capacity (crops)
  float *bufX = nullptr, *bufH = nullptr, *bufY = nullptr, *bufD = nullptr;
  // fused resample -> backbone: the crops between the two kernels (u8 grey levels, or fp32 in UT_REMAP_FLOAT mode)
  size_t crops_ws_floats = 0;
  float* crops_ws = nullptr;
  size_t wsb_crops = 0;   // phase-B capacity (crops)
  float *bufL2 = nullptr, *bufP = nullptr, *bufQ = nullptr, *bufBH = nullptr, *bufBD = nullptr;
  // head workspace
  size_t ws_samples = 0;
  ut::HeadBuffers hb{};
  size_t ws_skel = 0;
  // temporal state
  int slots_cap = 0, slots_used = 0;
  float *mem = nullptr, *prev_ext = nullptr;
  // per-launch device words, zeroed by one memset at the start of a call: [i] the tile queue of launch i of the call,
  // [kMaxCounters + i] the bits of the largest magnitude that launch stored (the activation scale of a split-fp16 consumer)
  unsigned* counters = nullptr;
  int counter_next = 0;
  // split-fp16 activation scales.  Tensor ids: 0 the stem's output, 1 + 2b the output of block b's first convolution, 2 + 2b
  // block b's output (b = 0 .. 11).  calib[t]: the bits of 2^kCalibHeadroom x the largest magnitude of tensor t over the
  // calibration crops (device words behind the per-launch words; never zeroed by begin_call).
  unsigned* calib = nullptr;
  unsigned* adapt_count = nullptr;  // UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE: split launches that adapted (ut_get_split_adaptations; both
                                    // lanes; the last of the 64 words at calib, so a calibration zeroes it)
  int scale_mode = UT_SPLIT_SCALE_CALIBRATED;
  bool calibrated = false;
  bool head_calibrated = false;     // ... including the regressor's tensors (needs at least two calibration crops)
  bool calibrating = false;         // the running backbone call is a calibration pass: dynamic scales, maxima merged into calib
  unsigned word_gen = 0;            // bumped by every zeroing of the words: a max word kept across launches is stale after it
  bool block_fusion = true;         // ut_set_block_fusion: split-fp16 mode - layer1's BasicBlocks and layer2's entry as one launch each, the
                                    // regressor's zero K slice skipped; both arithmetics - the fp32 1x1 convolutions on conv_pw.hip (run_pw)
  int resident_weights = 1;         // split-fp16 mode (ut_set_resident_weights): 1 conv_w4 wherever it applies, 0 the chunked kernels, 2 .. 7 A/B mixes
  // conv_w4 chains (run_conv, flush_chain): consecutive launches of conv_w4's stride-1 forms, each reading what the one before
  // wrote, wait here and go out as one launch in front of the next other launch on their stream
  std::vector<ut::ConvLaunch> chain;
  double chain_flops = 0;
  hipStream_t chain_stream = nullptr;
  bool call_split = false;          // the running backbone call uses the split-fp16 kernels (decided once per call)
  // index checks: device status words ([0] sticky errors, [1] per call), their pinned host mirror, the duplicate-slot
  // scratch (slots_cap ints, allocated with the temporal state) and the mode (UT_CHECK_*)
  int* status = nullptr;
  int* status_host = nullptr;
  int* slot_seen = nullptr;
  int check_mode = UT_CHECK_SYNC;
  // backbone lanes (ut_set_backbone_lanes): a large batch runs as two half-batches on two internal streams, so that
  // the tail of one lane's launch (workgroups that found the tile queue empty) is filled by the other lane's launch
  int lanes = 1;
  hipStream_t lane_stream[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // UT_CONV_FP32 (exact fp32 matrix instructions) or UT_CONV_SPLIT_F16 (conv_split.hip on the eligible layers)
  int conv_arith = UT_CONV_FP32;
  // latency mode (ut_set_latency_mode): launches with far fewer tiles than CUs split K across workgroups
  bool latency_mode = false;
  float* splitk_ws = nullptr;      // [splits][M][cout] partial sums
  size_t splitk_floats = 0;
  float* zero_bias = nullptr;      // 256 zeros
  // profiling
  bool profiling = false;
  std::vector<ProfEvent> prof;
};

namespace {

int fail(ut_handle h, int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof buf, "%s", what);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(h, x)                                            \
  do {                                                          \
    hipError_t e_ = (x);                                        \
    if (e_ != hipSuccess) return fail(h, UT_E_HIP, #x, e_);     \
  } while (0)

// Every entry that allocates or launches runs on the handle's device whatever the caller's current device is,
// and leaves the caller's current device as it found it.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {      // dev < 0: stay on the caller's current device
    if (dev < 0) return;
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = err == hipSuccess;
    }
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
#define ON_DEVICE_IF(h)                                        \
  DeviceScope scope_((h) ? (h)->device : -1);                  \
  if ((h) && scope_.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope_.err)
#define ON_DEVICE_OF(h)                 \
  DeviceScope scope_((h)->device);      \
  if (scope_.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope_.err)

// Status words for the stateless entry points (handle == NULL): one pair per device, created on first use.
struct DevStatus { int* dev = nullptr; int* host = nullptr; };
std::mutex g_status_mutex;
DevStatus g_status[64];

int stateless_status(int* device_out, DevStatus* out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail(nullptr, UT_E_HIP, "hipGetDevice", e);
  if (dev < 0 || dev >= 64) return fail(nullptr, UT_E_INVALID, "device index beyond 63");
  std::lock_guard<std::mutex> lock(g_status_mutex);
  DevStatus& st = g_status[dev];
  if (!st.dev) {
    void *d = nullptr, *hst = nullptr;
    if ((e = hipMalloc(&d, 2 * sizeof(int))) != hipSuccess) return fail(nullptr, UT_E_HIP, "hipMalloc", e);
    if ((e = hipHostMalloc(&hst, 2 * sizeof(int), hipHostMallocDefault)) != hipSuccess) {
      (void)hipFree(d);
      return fail(nullptr, UT_E_HIP, "hipHostMalloc", e);
    }
    if ((e = hipMemset(d, 0, 2 * sizeof(int))) != hipSuccess) return fail(nullptr, UT_E_HIP, "hipMemset", e);
    st.dev = (int*)d; st.host = (int*)hst;
  }
  *device_out = dev;
  *out = st;
  return UT_OK;
}

const char* status_message(int bits) {
  if (bits & ut::UT_SPLIT_RANGE)
    return "range check: an activation entering a split-fp16 convolution is an infinity or a NaN, or lies beyond the calibrated range "
           "of its layer (32 x the calibration maximum; ut_calibrate_split with representative crops, UT_SPLIT_SCALE_DYNAMIC or "
           "UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE)";
  if (bits & ut::UT_BAD_SRC_INDEX) return "index check: src_index outside [0, n_src_images)";
  if (bits & ut::UT_BAD_SAMPLE_RANGE) return "index check: sample_range rows must select 1 or 2 crops inside [0, n_crops]";
  if (bits & ut::UT_BAD_MEMORY_IDX) return "index check: memory_idx outside [0, n_slots)";
  if (bits & ut::UT_DUP_MEMORY_IDX) return "index check: memory_idx names one temporal slot twice";
  if (bits & ut::UT_BAD_HAND_IDX) return "index check: hand_idx must be 0 (left) or 1 (right)";
  return "index check: failed";
}

// Read the status words back into `host` (synchronises the stream) and fail with "<what>: <message>" when the sticky word
// holds an error; a non-zero sticky word is cleared.  host[1] keeps the per-call word for the caller.
int check_status(ut_handle h, int* dev, int* host, hipStream_t s, const char* what) {
  HIPCHK(h, hipMemcpyAsync(host, dev, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  const int sticky = host[0];
  if (sticky) HIPCHK(h, hipMemsetAsync(dev, 0, sizeof(int), s));
  if (sticky & ut::UT_STATUS_ERRORS) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, status_message(sticky));
    return fail(h, UT_E_INVALID, buf);
  }
  return UT_OK;
}

int upload_bytes(ut_handle h, const void* host, size_t bytes, void** dev) {
  void* d = nullptr;
  HIPCHK(h, hipMalloc(&d, bytes));
  h->allocs.push_back(d);
  HIPCHK(h, hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
  *dev = d;
  return UT_OK;
}

int upload(ut_handle h, const std::vector<float>& host, float** dev) {
  return upload_bytes(h, host.data(), host.size() * sizeof(float), (void**)dev);
}

// The weights arrive folded and laid out (ut_weights.h); everything below only copies them to the device.
int upload_conv(ut_handle h, ConvW& cw, const ut::PackedConv& pc) {
  static_cast<ut::ConvGeom&>(cw) = pc;
  cw.split_unscale = pc.split_unscale; cw.wsum_rows = pc.wsum_rows; cw.bias_max = pc.bias_max;
  int rc = upload(h, pc.wp, &cw.w);
  if (!rc && !pc.wfrag.empty()) rc = upload(h, pc.wfrag, &cw.w_frag);
  if (!rc && !pc.planes.empty()) rc = upload_bytes(h, pc.planes.data(), pc.planes.size() * sizeof(uint16_t), &cw.w_split);
  return rc ? rc : upload(h, pc.bp, &cw.bias);
}

// pw_ds: the shortcut also in conv_pw.hip's fragment order (layer4's entry)
int upload_block(ut_handle h, Block& b, const ut::FoldedBlock& fb, bool pw_ds = false) {
  int rc;
  const int cs = ut::round_up(fb.conv1.cout, 4);
  if ((rc = upload_conv(h, b.conv1, ut::pack_conv_host(fb.conv1, 3, fb.stride, cs)))) return rc;
  if ((rc = upload_conv(h, b.conv2, ut::pack_conv_host(fb.conv2, 3, 1, cs)))) return rc;
  b.has_ds = fb.has_ds;
  if (fb.has_ds && (rc = upload_conv(h, b.ds, ut::pack_conv_host(fb.ds, 1, fb.stride, cs, pw_ds)))) return rc;
  return UT_OK;
}

int upload_regressor(ut_handle h, Regressor& r, const ut::FoldedRegressor& fr) {
  r.c = fr.c; r.d = fr.d;
  int rc;
  for (int i = 0; i < 2; ++i)
    if ((rc = upload_block(h, r.blocks[i], fr.blocks[i])) || (rc = upload_block(h, r.blocks_split[i], fr.wide[i]))) return rc;
  // the wide form's real channels (76 or 72 of 128): its fourth 32-channel slice of K is zeros
  for (int i = 0; i < 2; ++i) {
    r.blocks_split[i].conv1.k_cin = ut::round_up(fr.blocks[i].conv1.cin, 32);
    r.blocks_split[i].conv2.k_cin = ut::round_up(fr.blocks[i].conv2.cin, 32);
  }
  if ((rc = upload(h, fr.w_out, &r.w_out))) return rc;
  return upload(h, fr.b_out, &r.b_out);
}

int dev_alloc(ut_handle h, float** p, size_t n_floats) {
  void* d = nullptr;
  HIPCHK(h, hipMalloc(&d, n_floats * sizeof(float)));
  h->allocs.push_back(d);
  *p = (float*)d;
  return UT_OK;
}

void dev_free(ut_handle h, void* p) {
  if (!p) return;
  for (size_t i = 0; i < h->allocs.size(); ++i)
    if (h->allocs[i] == p) { h->allocs.erase(h->allocs.begin() + i); break; }
  (void)hipFree(p);
}

// Regrow a set of workspace buffers to n units each (`bufs`: a buffer and its floats per unit) when *cap < n.  Launches in
// flight may still use the old buffers, hence the synchronise; *cap stays 0 until every allocation has succeeded.
int regrow(ut_handle h, size_t* cap, size_t n, std::initializer_list<std::pair<float**, size_t>> bufs) {
  if (n <= *cap) return UT_OK;
  HIPCHK(h, hipDeviceSynchronize());
  for (auto& b : bufs) { dev_free(h, *b.first); *b.first = nullptr; }
  *cap = 0;
  int rc;
  for (auto& b : bufs)
    if ((rc = dev_alloc(h, b.first, n * b.second))) return rc;
  *cap = n;
  return UT_OK;
}

int ensure_backbone_ws(ut_handle h, int crops) {
  const size_t big = 48 * 48 * 32, small = 24 * 24 * 64;
  return regrow(h, &h->ws_crops, crops, {{&h->bufX, big}, {&h->bufH, big}, {&h->bufY, big}, {&h->bufD, small}});
}

constexpr int PHASE_B_MAX = 8192;    // its input, the 24x24x64 map (147 KB per crop), must stay under 2^31 bytes: < 14563 crops

int ensure_phase_b_ws(ut_handle h, int crops) {
  const size_t l2 = 24 * 24 * 64, l3 = 12 * 12 * 128;
  return regrow(h, &h->wsb_crops, crops, {{&h->bufL2, l2}, {&h->bufP, l3}, {&h->bufQ, l3}, {&h->bufBH, l3}, {&h->bufBD, l3}});
}

int ensure_head_ws(ut_handle h, int samples, int n_skel) {
  ut::HeadBuffers& b = h->hb;
  const size_t r = 36 * ut::kRegSplitCh;
  int rc = regrow(h, &h->ws_samples, samples, {{&b.cat144, 36 * 144}, {&b.f108, 36 * 108}, {&b.f72a, 36 * 72}, {&b.f72b, 36 * 72},
                                                {&b.fused, 36 * 72}, {&b.t92a, 36 * 92}, {&b.t92b, 36 * 92}, {&b.regin, r},
                                                {&b.rega, r}, {&b.regb, r}});
  return rc ? rc : regrow(h, &h->ws_skel, n_skel, {{&b.skel, 36 * 4}});
}

int ensure_slots(ut_handle h, int slots, hipStream_t s) {
  if (slots <= h->slots_cap) return UT_OK;
  int cap = h->slots_cap ? h->slots_cap : 2;
  while (cap < slots) cap *= 2;
  float *nm = nullptr, *ne = nullptr, *seen = nullptr;
  int rc;
  if ((rc = dev_alloc(h, &nm, (size_t)cap * 36 * 18)) || (rc = dev_alloc(h, &ne, (size_t)cap * 16)) ||
      (rc = dev_alloc(h, &seen, (size_t)cap)))
    return rc;
  HIPCHK(h, hipMemsetAsync(nm, 0, (size_t)cap * 36 * 18 * sizeof(float), s));
  HIPCHK(h, hipMemsetAsync(ne, 0, (size_t)cap * 16 * sizeof(float), s));
  if (h->slots_cap) {
    HIPCHK(h, hipMemcpyAsync(nm, h->mem, (size_t)h->slots_cap * 36 * 18 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(ne, h->prev_ext, (size_t)h->slots_cap * 16 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    dev_free(h, h->mem);
    dev_free(h, h->prev_ext);
    dev_free(h, h->slot_seen);
  }
  h->mem = nm; h->prev_ext = ne; h->slot_seen = (int*)seen; h->slots_cap = cap;
  return UT_OK;
}

constexpr int kMaxCounters = 4096;
constexpr int kScaleTensors = 33;      // 25 of the backbone; 25 .. 28 the known-skeleton regressor's input, inner tensors and first block's output, 29 .. 32 the other regressor's
static_assert(kScaleTensors < 63, "the adaptation counter is the last of the 64 words at ut_context::calib");
constexpr int kCalibHeadroom = 4;      // calibrated scale words hold 2^4 x the calibration maximum: inputs up to 32 x that maximum
                                       // (the scale leaves another factor 2 under fp16's 65504) are inside the split's range

int flush_chain(ut_handle h);

// zero the per-launch words (tile queues, output maxima) used by the launches of one API call (stream ordered)
int begin_call(ut_handle h, hipStream_t s) {
  if (const int rc = flush_chain(h)) return rc;      // (a zeroing in mid-call: the collected launches own words)
  h->counter_next = 0;
  ++h->word_gen;
  HIPCHK(h, ut::launch_zero_words(h->counters, 2 * kMaxCounters, s));      // a kernel, not a memset node: see launch_zero_words
  return UT_OK;
}

// The lease on the per-launch words: the next n launches take theirs (take_word) from one zeroing, so that a word handed from one
// of them to the next stays live.  With fewer than n left the words are zeroed (in stream order, behind the earlier launches) and
// handed out again; *zeroed (optional) reports it: every max word an earlier launch of the call left is stale then.
int lease_words(ut_handle h, hipStream_t s, int n, bool* zeroed = nullptr) {
  const bool full = h->counter_next + n > kMaxCounters;
  if (zeroed) *zeroed = full;
  return full ? begin_call(h, s) : UT_OK;
}
int take_word(ut_handle h) { return h->counter_next++; }      // index of the next launch's words, inside a lease

// The scale word a split-fp16 consumer of tensor `tid` reads, and the word it guards against: calibrated mode - the handle's
// calibrated word, guarded by the word the producer left in this call (may be null); adaptive mode - the same, and the consumer
// takes the producer's word instead when it lies outside the calibrated band (ut_kernels.h::split_act_scale); dynamic mode and
// calibration passes - the producer's word itself (null: no scale, the launch stays on the fp32 instruction).
struct ScaleRef { const unsigned* word = nullptr; const unsigned* obs = nullptr; int adaptive = 0; unsigned* adapt_count = nullptr; };
ScaleRef scale_for(ut_handle h, int tid, const unsigned* producer_word) {
  ScaleRef r;
  if (!h->call_split || h->latency_mode || tid < 0 || tid >= kScaleTensors) return r;
  if (h->calibrating || h->scale_mode == UT_SPLIT_SCALE_DYNAMIC) r.word = producer_word;
  else { r.word = h->calib + tid; r.obs = producer_word; }
  if (!h->calibrating && h->scale_mode == UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE && r.obs) { r.adaptive = 1; r.adapt_count = h->adapt_count; }
  return r;
}
// the scale fields that ConvLaunch, BlockLaunch and Stride2Launch share
template <class Launch>
void set_scale(Launch& l, const ScaleRef& sr, int* status) {
  l.in_max = sr.word; l.in_obs = sr.obs; l.split_adaptive = sr.adaptive; l.adapt_count = sr.adapt_count; l.status = status;
}
// One convolution launch (`launch()` enqueues kernel `what`).  A calibration pass first folds the producer's word of the
// input tensor `in_tid` into its calibrated word; while the handle profiles, two events time the launch, kept with its flops
// and kind (ProfEvent).  (A calibration pass never profiles: calibrate_split turns profiling off.)
template <class Launch>
int bracket_launch(ut_handle h, hipStream_t s, int in_tid, const unsigned* in_max, double flops, int kind, const char* what,
                   Launch launch, int convs = 1) {
  if (const int rc = flush_chain(h)) return rc;      // in stream order: what was collected goes first
  if (h->calibrating && in_max && in_tid >= 0 && in_tid < kScaleTensors) HIPCHK(h, ut::launch_merge_max(h->calib + in_tid, in_max, s));
  ProfEvent pe{nullptr, nullptr, flops, kind, convs};
  if (h->profiling) {
    HIPCHK(h, hipEventCreateWithFlags(&pe.a, hipEventDisableSystemFence));   // timing only: no system-scope flush per kernel
    HIPCHK(h, hipEventCreateWithFlags(&pe.b, hipEventDisableSystemFence));
    HIPCHK(h, hipEventRecord(pe.a, s));
  }
  const hipError_t e = launch();
  if (e != hipSuccess) return fail(h, UT_E_HIP, what, e);
  if (h->profiling) {
    HIPCHK(h, hipEventRecord(pe.b, s));
    h->prof.push_back(pe);
  }
  return UT_OK;
}

// The collected conv_w4 launches (run_conv) as one launch - a single one as itself -, bracketed as ONE launch of kind 1 with the
// layers' summed flops.  Called in front of every other launch that could follow them on their stream, and where a pass or the
// head ends.
int flush_chain(ut_handle h) {
  if (h->chain.empty()) return UT_OK;
  std::vector<ut::ConvLaunch> layers;
  layers.swap(h->chain);
  const double flops = h->chain_flops;
  h->chain_flops = 0;
  hipStream_t s = h->chain_stream;
  if (layers.size() == 1)
    return bracket_launch(h, s, -1, nullptr, flops, 1, "conv_w4", [&] { return ut::launch_conv_w4(layers[0], s); });
  return bracket_launch(h, s, -1, nullptr, flops, 1, "conv_w4 chain",
                        [&] { return ut::launch_conv_w4_chain(layers.data(), (int)layers.size(), s); }, (int)layers.size());
}

// in_max: the max word of the launch that produced `in` (null: unknown); in_tid: the tensor id of `in` (< 0: not a tensor of the
// split-fp16 path - the launch stays on the fp32 instruction);
// *out_max (optional): receives this launch's max word when it ran a kernel that leaves one, else null
int run_conv(ut_handle h, const ConvW& cw, const float* in, const float* res, float* out, int n_img, int H, int W,
             bool relu, bool nchw, hipStream_t s, const unsigned* in_max = nullptr, unsigned** out_max = nullptr, int in_tid = -1) {
  if (out_max) *out_max = nullptr;
  ut::ConvLaunch c{};
  c.in = in; c.w = cw.w; c.bias = cw.bias; c.res = res; c.out = out;
  c.n_img = n_img; c.H = H; c.W = W; c.cin = cw.cin_pad;
  c.Ho = (H + 2 * cw.pad - cw.ksize) / cw.stride + 1;
  c.Wo = (W + 2 * cw.pad - cw.ksize) / cw.stride + 1;
  c.cout_store = cw.cout_store; c.cout_pad = cw.cout_pad;
  c.k_total = cw.k_total; c.k_pad = cw.k_pad; c.cslice = cw.cslice;
  c.k_cin = h->block_fusion && cw.k_cin < cw.cin_pad ? cw.k_cin : 0;     // (the switch off: every convolution walks its whole K)
  c.ksize = cw.ksize; c.stride = cw.stride; c.pad = cw.pad;
  c.relu = relu; c.out_nchw = nchw;
  c.device = h->device; c.num_cu = h->num_cu; c.no_resident = ut::kResidentKinds[h->resident_weights];
  bool zeroed = false;
  int rc = lease_words(h, s, 1, &zeroed);
  if (rc) return rc;
  if (zeroed) in_max = nullptr;      // zeroed in mid-call: the producer's word is gone
  const int word = take_word(h);
  c.tile_counter = h->counters + word;
  // Latency mode: a convolution of a few crops has far fewer 64x64 tiles than the chip has CUs and every workgroup
  // walks all of K alone (a layer-4 conv of 4 crops: 12 tiles x 72 chunks).  Cut K into S equal chunk ranges (S the
  // largest divisor of the chunk count that leaves >= 6 chunks per range and <= one workgroup per CU), let S x tiles
  // workgroups write partial sums and add them in a fixed order afterwards.  Deterministic, but the summation order
  // differs from the unsplit kernel's: results agree with it to fp32 rounding, not bit for bit - hence opt-in.
  int splits = 1;
  if (h->latency_mode && !nchw && cw.cout_store % 4 == 0) {
    const long m = (long)n_img * c.Ho * c.Wo;
    const long tiles64 = ((m + 63) / 64) * ((cw.cout_store + 63) / 64);
    const int chunks = cw.k_pad / 32;
    for (int sp = 2; sp <= chunks / 6; ++sp)
      if (chunks % sp == 0 && tiles64 * sp <= (long)h->num_cu && (size_t)sp * m * cw.cout_store <= h->splitk_floats) splits = sp;
  }
  if (h->latency_mode) c.splits = 1;
  if (splits > 1) {
    ut::ConvLaunch part = c;
    part.bias = h->zero_bias; part.res = nullptr; part.relu = 0; part.out = h->splitk_ws; part.splits = splits;
    HIPCHK(h, ut::launch_conv_igemm(part, s));
    HIPCHK(h, ut::launch_splitk_finish(h->splitk_ws, splits, n_img * c.Ho * c.Wo, cw.cout_store, cw.bias, res, out,
                                       relu ? 1 : 0, s));
    return UT_OK;
  }
  // split-fp16 arithmetic: decided once per backbone call (run_backbone), for every eligible layer of the call whose
  // producer left a max word; everything else - the head, and every launch in latency mode - stays on the fp32 instruction
  const ScaleRef sr = scale_for(h, in_tid, in_max);
  c.w_split = sr.word ? cw.w_split : nullptr;
  c.split_unscale = cw.split_unscale;
  set_scale(c, sr, h->status);
  const ut::ConvKernel kernel = ut::choose_conv(c);
  const int kind = c.w_split && kernel != ut::CONV_IGEMM ? 1 : 0;      // every other kernel computes in split-fp16 when it has the planes
  if (kind) {
    c.out_max = h->counters + kMaxCounters + word;
    if (out_max) *out_max = c.out_max;
  }
  const double flops = cw.flops_per_pixel * (double)n_img * c.Ho * c.Wo;
  // conv_w4's stride-1 forms under a calibrated scale that no launch adapts: collected, and issued with the launches that follow
  // it as one chain (flush_chain).  Everything else - and kind 7 of ut_set_resident_weights - launches now, behind what was collected.
  const ut::W4Form form = kernel == ut::CONV_W4 ? ut::conv_w4_form(c) : ut::W4_NONE;
  if (kind && (form == ut::W4_TILES128 || form == ut::W4_MAP24) && !(c.no_resident & ut::NO_W4_CHAIN) && h->block_fusion &&
      !h->calibrating && !h->latency_mode && h->scale_mode == UT_SPLIT_SCALE_CALIBRATED && c.in_max && !c.split_adaptive &&
      ut::conv_w4_chain_fills(c)) {
    if (!h->chain.empty() && (h->chain_stream != s || (int)h->chain.size() == ut::W4_MAX_CHAIN || !ut::conv_w4_chainable(h->chain.back(), c)))
      if ((rc = flush_chain(h))) return rc;
    h->chain.push_back(c);
    h->chain_flops += flops;
    h->chain_stream = s;
    return UT_OK;
  }
  return bracket_launch(h, s, kind ? in_tid : -1, in_max, flops, kind,
                        ut::kConvKernelName[kernel], [&] { return ut::launch_conv_on(kernel, c, s); });
}

// 1x1 convolutions without residual, alone or as a chain whose intermediates nothing else reads, in one streaming launch
// (conv_pw.hip): the bits of the same layers through run_conv, in either convolution arithmetic (these layers are fp32 in both).
// Taken while the handle's fusion switch is on and outside latency mode (whose split-K path stays as it is); *done = false:
// not taken, the caller launches the layers one by one.
int run_pw(ut_handle h, std::initializer_list<const ConvW*> layers, std::initializer_list<bool> relus, const float* in, float* out,
           int n_img, int H, int W, bool nchw, hipStream_t s, bool* done) {
  *done = false;
  if (!h->block_fusion || h->latency_mode) return UT_OK;
  ut::PwLaunch c{};
  double flops = 0;
  const ConvW& first = **layers.begin();
  c.in = in; c.out = out; c.n_img = n_img; c.H = H; c.W = W; c.cin = first.cin_pad; c.stride = first.stride;
  c.Ho = (H - 1) / first.stride + 1; c.Wo = (W - 1) / first.stride + 1;
  c.out_nchw = nchw; c.num_cu = h->num_cu;
  auto relu = relus.begin();
  for (const ConvW* cw : layers) {
    if (cw->ksize != 1 || cw->pad != 0 || !cw->w_frag || (c.n_layers > 0 && cw->stride != 1)) return UT_OK;
    c.layer[c.n_layers++] = ut::PwLayer{cw->w_frag, cw->bias, cw->k_pad, cw->cout_store, cw->cout_pad, *relu++ ? 1 : 0};
    c.cout_store = cw->cout_store;
    flops += cw->flops_per_pixel * (double)n_img * c.Ho * c.Wo;
  }
  if (!ut::conv_pw_applicable(c)) return UT_OK;
  *done = true;
  return bracket_launch(h, s, -1, nullptr, flops, 0, "launch_conv_pw", [&] { return ut::launch_conv_pw(c, s); });
}

// relu(bn2(conv2(relu(bn1(conv1 x)))) + (downsample(x) | x))   lib/models/backbone_resnet.py:56-72
// x_max: the max word of x's producer (or null); *y_max (optional): the word of the block's output;
// x_tid / mid_tid: the scale-tensor ids of x and of conv1's output (backbone block b: 2 b, 2 b + 1; < 0: no split-fp16 path)
int run_block(ut_handle h, const Block& b, const float* x, float* tmp, float* dsbuf, float* y, int n_img, int H,
              int W, hipStream_t s, const unsigned* x_max = nullptr, unsigned** y_max = nullptr, int x_tid = -1, int mid_tid = -1) {
  int rc;
  if (y_max) *y_max = nullptr;
  // the words of one block (at most three launches): the word conv1 hands to conv2 stays live between the two
  bool zeroed = false;
  if ((rc = lease_words(h, s, 8, &zeroed))) return rc;
  if (zeroed) x_max = nullptr;
  const ScaleRef xs = scale_for(h, x_tid, x_max);
  // layer1 in split-fp16 mode: the whole block in one launch, the intermediate stays in LDS (conv_block32.hip)
  if (h->block_fusion && xs.word && !b.has_ds && b.conv1.w_split && b.conv2.w_split && b.conv1.stride == 1 &&
      b.conv1.cin_pad == 32 && b.conv1.cout_store == 32 && b.conv2.cout_store == 32) {
    ut::BlockLaunch bl{};
    bl.in = x; bl.out = y; bl.w1_split = b.conv1.w_split; bl.w2_split = b.conv2.w_split;
    bl.unscale_w1 = b.conv1.split_unscale; bl.unscale_w2 = b.conv2.split_unscale;
    bl.bias1 = b.conv1.bias; bl.bias2 = b.conv2.bias;
    bl.wsum1 = b.conv1.wsum_rows; bl.bmax1 = b.conv1.bias_max;
    set_scale(bl, xs, h->status);
    bl.n_img = n_img; bl.H = H; bl.W = W; bl.device = h->device; bl.num_cu = h->num_cu;
    bl.tile_counter = h->counters + h->counter_next;      // the word it takes if it applies
    if (ut::conv_block32_applicable(bl)) {
      bl.out_max = h->counters + kMaxCounters + take_word(h);
      const double flops = (b.conv1.flops_per_pixel + b.conv2.flops_per_pixel) * (double)n_img * H * W;
      if ((rc = bracket_launch(h, s, x_tid, x_max, flops, 1, "conv_block32", [&] { return ut::launch_conv_block32(bl, s); })))
        return rc;
      if (y_max) *y_max = bl.out_max;
      return UT_OK;
    }
  }
  // layer2's entry in split-fp16 mode: the stride-2 3x3 and the 1x1 shortcut from one pass over x (conv_c32s2.hip)
  if (h->block_fusion && xs.word && b.has_ds && b.conv1.w_split && b.ds.w_split && b.conv2.w_split &&
      b.conv1.stride == 2 && b.conv1.cin_pad == 32 && b.conv1.cout_store == 64 && b.ds.cout_store == 64 && dsbuf) {
    ut::Stride2Launch sl{};
    sl.in = x; sl.out1 = tmp; sl.out2 = dsbuf; sl.w1_split = b.conv1.w_split; sl.wd_split = b.ds.w_split;
    sl.unscale1 = b.conv1.split_unscale; sl.unscale_d = b.ds.split_unscale;
    sl.bias1 = b.conv1.bias; sl.bias_d = b.ds.bias;
    set_scale(sl, xs, h->status);
    sl.n_img = n_img; sl.H = H; sl.W = W; sl.device = h->device; sl.num_cu = h->num_cu;
    if (ut::conv_c32s2_applicable(sl)) {
      sl.out1_max = h->counters + kMaxCounters + take_word(h);
      const double flops = (b.conv1.flops_per_pixel + b.ds.flops_per_pixel) * (double)n_img * (H / 2) * (W / 2);
      if ((rc = bracket_launch(h, s, x_tid, x_max, flops, 1, "conv_c32s2", [&] { return ut::launch_conv_c32s2(sl, s); })))
        return rc;
      return run_conv(h, b.conv2, tmp, dsbuf, y, n_img, H / 2, W / 2, true, false, s, sl.out1_max, y_max, mid_tid);
    }
  }
  unsigned* tmp_max = nullptr;
  if ((rc = run_conv(h, b.conv1, x, nullptr, tmp, n_img, H, W, true, false, s, x_max, &tmp_max, x_tid))) return rc;
  const int Ho = (H + 2 - 3) / b.conv1.stride + 1, Wo = (W + 2 - 3) / b.conv1.stride + 1;
  const float* res = x;
  if (b.has_ds) {
    bool streamed = false;
    if ((rc = run_pw(h, {&b.ds}, {false}, x, dsbuf, n_img, H, W, false, s, &streamed))) return rc;
    if (!streamed && (rc = run_conv(h, b.ds, x, nullptr, dsbuf, n_img, H, W, false, false, s))) return rc;
    res = dsbuf;
  }
  return run_conv(h, b.conv2, tmp, res, y, n_img, Ho, Wo, true, false, s, tmp_max, y_max, mid_tid);
}

// destroy the timing events of the launches profiled so far (the handle's device must be current)
void prof_clear(ut_handle h) {
  for (auto& pe : h->prof) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
  h->prof.clear();
}

// end profiling: per kind (ProfEvent::kind), the summed times, launch counts and flops of the launches since ut_profile_begin
// (a conv_w4 chain: one time, its layers' flops, and one count per layer - the count stays the number of convolutions)
int prof_reduce(ut_handle h, hipStream_t s, double ms[2], int64_t launches[2], double flops[2]) {
  h->profiling = false;
  HIPCHK(h, hipStreamSynchronize(s));
  for (int k = 0; k < 2; ++k) { ms[k] = 0; launches[k] = 0; flops[k] = 0; }
  for (auto& pe : h->prof) {
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, pe.a, pe.b));
    const int k = pe.kind ? 1 : 0;
    ms[k] += t; flops[k] += pe.flops; launches[k] += pe.convs;
  }
  prof_clear(h);
  return UT_OK;
}

}  // namespace

extern "C" {

size_t ut_weight_blob_floats(void) { return UT_WEIGHT_BLOB_FLOATS; }

const char* ut_last_error(ut_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ut_canonical_backbone_weights(const float* blob, size_t n_floats, float* out, size_t out_floats, size_t* n_out) {
  if (!blob || !n_out) return fail(nullptr, UT_E_INVALID, "ut_canonical_backbone_weights: null argument");
  if (n_floats != UT_WEIGHT_BLOB_FLOATS) return fail(nullptr, UT_E_WEIGHTS, "ut_canonical_backbone_weights: weight blob has the wrong length");
  ut::FoldedNetwork net;
  if (!ut::fold_network(blob, n_floats, net)) return fail(nullptr, UT_E_WEIGHTS, "weight blob length does not match the architecture");
  const ut::FoldedBackbone& fbb = net.backbone;
  std::vector<const ut::Folded*> all = {&fbb.stem};
  for (const ut::FoldedBlock& b : fbb.fb) {
    all.push_back(&b.conv1); all.push_back(&b.conv2);
    if (b.has_ds) all.push_back(&b.ds);
  }
  all.push_back(&fbb.proj);
  size_t n = 0;
  for (const ut::Folded* f : all) n += f->w.size() + f->b.size();
  *n_out = n;
  if (!out) return UT_OK;
  if (out_floats < n) return fail(nullptr, UT_E_INVALID, "ut_canonical_backbone_weights: output too small");
  for (const ut::Folded* f : all) {
    memcpy(out, f->w.data(), f->w.size() * sizeof(float)); out += f->w.size();
    memcpy(out, f->b.data(), f->b.size() * sizeof(float)); out += f->b.size();
  }
  return UT_OK;
}

int ut_create(int device, const float* blob, size_t n_floats, ut_handle* out) {
  if (!blob || !out) return fail(nullptr, UT_E_INVALID, "ut_create: null argument");
  if (n_floats != UT_WEIGHT_BLOB_FLOATS) return fail(nullptr, UT_E_WEIGHTS, "ut_create: weight blob has the wrong length");
  ut::FoldedNetwork net;      // the whole blob, folded on the host, before the handle owns any device memory
  if (!ut::fold_network(blob, n_floats, net)) return fail(nullptr, UT_E_WEIGHTS, "weight blob length does not match the architecture");
  DeviceScope scope(device);          // the caller's current device is restored on return
  if (scope.err != hipSuccess) return fail(nullptr, UT_E_HIP, "hipSetDevice", scope.err);
  ut_handle h = new ut_context();
  h->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->num_cu = cus;
  }
  int rc = UT_OK;
  do {
    { float* cnt = nullptr; if ((rc = dev_alloc(h, &cnt, 2 * kMaxCounters + 64))) break; h->counters = (unsigned*)cnt;
      h->calib = h->counters + 2 * kMaxCounters;
      h->adapt_count = h->calib + 63;      // behind the kScaleTensors words: zeroed with them by a calibration
      hipError_t e1 = hipMemset(h->calib, 0, 64 * sizeof(unsigned));
      if (e1 != hipSuccess) { rc = fail(h, UT_E_HIP, "calibration words", e1); break; } }
    { float* st = nullptr; if ((rc = dev_alloc(h, &st, 2))) break; h->status = (int*)st;
      hipError_t e2 = hipMemset(h->status, 0, 2 * sizeof(int));
      if (e2 == hipSuccess) e2 = hipHostMalloc((void**)&h->status_host, 2 * sizeof(int), hipHostMallocDefault);
      if (e2 != hipSuccess) { rc = fail(h, UT_E_HIP, "status words", e2); break; } }
    const ut::FoldedBackbone& fbb = net.backbone;
    if ((rc = upload(h, fbb.stem.w, &h->stem_w)) || (rc = upload(h, fbb.stem.b, &h->stem_b))) break;
    for (int b = 0; b < 12 && !rc; ++b) rc = upload_block(h, h->bb[b], fbb.fb[b], b == 10);
    if (rc) break;
    if ((rc = upload_conv(h, h->proj, ut::pack_conv_host(fbb.proj, 1, 1, 72, true)))) break;
    if ((rc = upload_conv(h, h->fus0, ut::pack_conv_host(net.fusion[0], 1, 1, 108, true))) ||
        (rc = upload_conv(h, h->fus1, ut::pack_conv_host(net.fusion[1], 1, 1, 72, true))) ||
        (rc = upload_conv(h, h->fus2, ut::pack_conv_host(net.fusion[2], 1, 1, 72, true)))) break;
    // the temporal block's 90 channels live on a 92-channel padded layout
    for (int i = 0; i < 3 && !rc; ++i) rc = upload_conv(h, h->tmp[i], ut::pack_conv_host(net.temporal[i], 1, 1, 92, true));
    if (rc) break;
    if ((rc = upload(h, net.skel_w, &h->skel_w)) || (rc = upload(h, net.skel_b, &h->skel_b)) ||
        (rc = upload(h, net.skel_scale, &h->skel_scale)) || (rc = upload(h, net.skel_shift, &h->skel_shift))) break;
    if ((rc = upload_regressor(h, h->reg_k, net.reg_k))) break;
    rc = upload_regressor(h, h->reg_u, net.reg_u);
  } while (0);
  if (rc) {
    g_create_error = h->err;
    ut_destroy(h);
    return rc;
  }
  *out = h;
  return UT_OK;
}

int ut_destroy(ut_handle h) {
  if (!h) return UT_OK;
  DeviceScope scope(h->device);
  (void)hipDeviceSynchronize();
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->status_host) (void)hipHostFree(h->status_host);
  for (int i = 0; i < 2; ++i) {
    if (h->lane_stream[i]) (void)hipStreamDestroy(h->lane_stream[i]);
    if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  prof_clear(h);
  delete h;
  return UT_OK;
}

int ut_set_backbone_chunk(ut_handle h, int crops_per_pass) {
  if (!h || crops_per_pass < 0) return fail(h, UT_E_INVALID, "ut_set_backbone_chunk: bad argument");
  if (crops_per_pass > kMaxChunk) return fail(h, UT_E_INVALID, "ut_set_backbone_chunk: at most 7281 crops per pass (32-bit offsets)");
  h->chunk = crops_per_pass == 0 ? kDefaultChunk : crops_per_pass;
  return UT_OK;
}

int ut_reserve(ut_handle h, int max_crops, int max_samples, int max_slots) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  int rc;
  int c = max_crops < h->chunk ? max_crops : h->chunk;
  if (c > 0 && (rc = ensure_backbone_ws(h, c))) return rc;
  int cb = max_crops < PHASE_B_MAX ? max_crops : PHASE_B_MAX;
  if (cb > 0 && (rc = ensure_phase_b_ws(h, cb))) return rc;
  if (max_samples > 0 && (rc = ensure_head_ws(h, max_samples, max_samples))) return rc;
  if (max_slots > 0 && (rc = ensure_slots(h, max_slots, 0))) return rc;
  if (max_crops > 0 && (rc = regrow(h, &h->crops_ws_floats, (size_t)max_crops * 96 * 96, {{&h->crops_ws, 1}}))) return rc;
  return UT_OK;
}

int ut_warp_crops(ut_handle h, const uint8_t* src, int n_src_images, int src_h, int src_w, const double* cam_params,
                  const double* crop_params, const int32_t* src_index, int n_crops, int remap_mode, float* out,
                  void* stream) {
  // stateless: h may be NULL (then the call runs on the caller's current device and always checks synchronously)
  if (n_crops == 0) return UT_OK;
  if (!src || !cam_params || !crop_params || !src_index || !out || n_crops < 0 || src_h <= 0 || src_w <= 0 ||
      n_src_images <= 0 || (remap_mode != UT_REMAP_CV2_FIXED && remap_mode != UT_REMAP_FLOAT))
    return fail(h, UT_E_INVALID, "ut_warp_crops: bad argument");
  hipStream_t s = (hipStream_t)stream;
  int *st_dev = nullptr, *st_host = nullptr, mode = UT_CHECK_SYNC, dev = 0;
  if (h) { st_dev = h->status; st_host = h->status_host; mode = h->check_mode; dev = h->device; }
  else {
    DevStatus st;
    int rc = stateless_status(&dev, &st);
    if (rc) return rc;
    st_dev = st.dev; st_host = st.host;
  }
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  HIPCHK(h, ut::launch_warp(src, n_src_images, src_h, src_w, cam_params, crop_params, src_index, n_crops, remap_mode,
                            out, nullptr, st_dev, s));
  return mode == UT_CHECK_SYNC ? check_status(h, st_dev, st_host, s, "ut_warp_crops") : UT_OK;
}

extern "C" int ut_warp_map(const double* cam_params, const double* crop_params, const int32_t* src_index, int n_src_images,
                           int n_crops, float* out_map, void* stream) {
  if (n_crops == 0) return UT_OK;
  if (!cam_params || !crop_params || !src_index || !out_map || n_crops < 0 || n_src_images <= 0)
    return fail(nullptr, UT_E_INVALID, "ut_warp_map: bad argument");
  HIPCHK(nullptr, ut::launch_warp_map(cam_params, crop_params, src_index, n_src_images, n_crops, out_map, (hipStream_t)stream));
  return UT_OK;
}

// stem launch; *out_max receives its max word when the call runs the split-fp16 kernels
static int run_stem(ut_handle h, const float* crops, const uint8_t* crops_u8, float* out, int n, hipStream_t st,
                    unsigned** out_max) {
  *out_max = nullptr;
  if (const int rc = flush_chain(h)) return rc;
  if (h->call_split && !h->latency_mode) {
    const int rc = lease_words(h, st, 1);
    if (rc) return rc;
    *out_max = h->counters + kMaxCounters + take_word(h);
  }
  if (crops_u8) HIPCHK(h, ut::launch_stem_u8(crops_u8, h->stem_w, h->stem_b, out, n, *out_max, st));
  else HIPCHK(h, ut::launch_stem(crops, h->stem_w, h->stem_b, out, n, *out_max, st));
  return UT_OK;
}

// Crops c0 .. c0 + n - 1 of a call (fp32 `crops` or u8 `crops_u8`) through stem .. projection into their rows of `feat` on
// stream s, in the workspace slices that start at crop `off`.
static int backbone_pass_launches(ut_handle h, const float* crops, const uint8_t* crops_u8, float* feat, int c0, int n, int off,
                                  int chunk, hipStream_t s);
static int backbone_pass(ut_handle h, const float* crops, const uint8_t* crops_u8, float* feat, int c0, int n, int off,
                         int chunk, hipStream_t s) {
  int rc = backbone_pass_launches(h, crops, crops_u8, feat, c0, n, off, chunk, s);
  if (!rc) rc = flush_chain(h);      // (the projection has flushed layer4's chain already)
  if (rc) { h->chain.clear(); h->chain_flops = 0; }      // a failed pass leaves nothing collected
  return rc;
}
static int backbone_pass_launches(ut_handle h, const float* crops, const uint8_t* crops_u8, float* feat, int c0, int n, int off,
                                  int chunk, hipStream_t s) {
  int rc;
  const size_t a48 = (size_t)off * 48 * 48 * 32, a24 = (size_t)off * 24 * 24 * 64, a12 = (size_t)off * 12 * 12 * 128;
  // the words of one pass (<= 2 x 22 + 16 launches) come from one zeroing, so that none of them is recycled while live
  if ((rc = lease_words(h, s, 256))) return rc;
  // ---- phase A: stem + layer1 (48x48x32) + layer2 (24x24x64), `chunk` crops per pass
  unsigned* l2_max = nullptr;      // max word of bufL2: the passes' words merged when phase A took more than one pass
  const unsigned l2_gen = h->word_gen;
  for (int done = 0; done < n; done += chunk) {
    const int m = n - done < chunk ? n - done : chunk;
    const size_t first = (size_t)(c0 + done) * 96 * 96;
    unsigned* xm = nullptr;
    if ((rc = run_stem(h, crops ? crops + first : nullptr, crops_u8 ? crops_u8 + first : nullptr, h->bufX + a48, m, s, &xm))) return rc;
    float *x = h->bufX + a48, *y = h->bufY + a48;
    int hw = 48;
    for (int b = 0; b < 5; ++b) {
      float* dst = b == 4 ? h->bufL2 + a24 + (size_t)done * 24 * 24 * 64 : y;
      if ((rc = run_block(h, h->bb[b], x, h->bufH + a48, h->bufD + a24, dst, m, hw, hw, s, xm, &xm, 2 * b, 2 * b + 1))) return rc;
      hw = (hw + 2 - 3) / h->bb[b].conv1.stride + 1;
      float* t = x; x = y; y = t;
    }
    if ((rc = flush_chain(h))) return rc;      // (layer2's chain: its last word is read next)
    if (done == 0) l2_max = xm;
    else if (l2_max && xm) HIPCHK(h, ut::launch_merge_max(l2_max, xm, s));
    else l2_max = nullptr;
  }
  // ---- phase B: layer3 (12x12x128) + layer4 (6x6x256) + projection over the whole sub-batch
  const float* x = h->bufL2 + a24;
  float *y = h->bufP + a12, *other = h->bufQ + a12;
  int hw = 24;
  unsigned* xm = l2_gen == h->word_gen ? l2_max : nullptr;
  for (int b = 5; b < 12; ++b) {
    if ((rc = run_block(h, h->bb[b], x, h->bufBH + a12, h->bufBD + a12, y, n, hw, hw, s, xm, &xm, 2 * b, 2 * b + 1))) return rc;
    hw = (hw + 2 - 3) / h->bb[b].conv1.stride + 1;
    x = y;
    float* t = y; y = other; other = t;
  }
  // projection 256 -> 72, written NCHW like the reference (lib/models/model_utils.py:134)
  bool streamed = false;
  if ((rc = run_pw(h, {&h->proj}, {false}, x, feat + (size_t)c0 * 72 * 36, n, 6, 6, true, s, &streamed)) || streamed) return rc;
  return run_conv(h, h->proj, x, nullptr, feat + (size_t)c0 * 72 * 36, n, 6, 6, false, true, s);
}

// stem .. projection over crops given as fp32 (crops) or as u8 grey levels (crops_u8)
static int run_backbone(ut_handle h, const float* crops, const uint8_t* crops_u8, int n_crops, float* feat, hipStream_t s) {
  int rc;
  const int chunk = n_crops < h->chunk ? n_crops : h->chunk;
  if ((rc = ensure_backbone_ws(h, chunk))) return rc;
  const int pass_b = n_crops < PHASE_B_MAX ? n_crops : PHASE_B_MAX;
  if ((rc = ensure_phase_b_ws(h, pass_b))) return rc;
  if ((rc = begin_call(h, s))) return rc;
  // One arithmetic per call, for every eligible layer of it: the split-fp16 kernels when the batch fills the chip with
  // their 256-row tiles down to the 6x6 maps (512 crops = 72 row tiles x 2 column tiles at layer4), else exact fp32.
  h->call_split = h->conv_arith == UT_CONV_SPLIT_F16_ALWAYS || (h->conv_arith == UT_CONV_SPLIT_F16 && n_crops >= 2 * h->num_cu);
  // ---- two lanes: the batch fits one pass of both phases and is big enough for two full-chip half-batches.  Every
  // launch is a persistent grid that drains a tile queue; its last round leaves workgroup slots idle for up to a tile
  // time (70-140 us of a 1.3 ms launch).  Frames are independent, so the two halves run the same launch sequence on
  // two streams and each one's idle slots are taken by the other's workgroups.  Same kernels on the same crops: the
  // results are bit-identical to the single-stream order.  (Not while profiling: per-launch event times would overlap.)
  if (h->lanes == 2 && !h->profiling && n_crops <= chunk && n_crops <= pass_b && n_crops >= 1024) {
    if (!h->lane_stream[0]) {
      for (int i = 0; i < 2; ++i) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->lane_stream[i], hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
      }
      HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    }
    HIPCHK(h, hipEventRecord(h->ev_fork, s));
    const int n0 = n_crops / 2;
    for (int i = 0; i < 2; ++i) {
      const int off = i ? n0 : 0, n = i ? n_crops - n0 : n0;
      HIPCHK(h, hipStreamWaitEvent(h->lane_stream[i], h->ev_fork, 0));
      if ((rc = backbone_pass(h, crops, crops_u8, feat, off, n, off, chunk, h->lane_stream[i]))) return rc;
      HIPCHK(h, hipEventRecord(h->ev_join[i], h->lane_stream[i]));
    }
    for (int i = 0; i < 2; ++i) HIPCHK(h, hipStreamWaitEvent(s, h->ev_join[i], 0));
    return UT_OK;
  }
  for (int base = 0; base < n_crops; base += pass_b) {
    const int nb = n_crops - base < pass_b ? n_crops - base : pass_b;
    if ((rc = backbone_pass(h, crops, crops_u8, feat, base, nb, 0, chunk, s))) return rc;
  }
  return UT_OK;
}

static int run_head(ut_handle h, const ut::HeadArgs& a, const float* skel, int n_skel, int mode, float* out_pose, float* out_raw,
                    hipStream_t s);

// Calibration of the regressor's four tensors (per regress mode): the head on the calibration crops' features, paired into two-view
// samples with canned cameras (f = 130 px, the second view 6 cm to the side), zero temporal memory in scratch state, a zero skeleton.
static int calibrate_head(ut_handle h, const float* feat, int n_crops, hipStream_t s) {
  const int S = n_crops / 2;
  int rc = ensure_head_ws(h, S, 1);
  if (rc) return rc;
  // one scratch allocation: [intrinsics 2S x 9 | extrinsics 2S x 16 | skeleton 132 | mem S x 648 | prev_ext S x 16 | pose S x 60 | raw S x 64]
  // floats, then [sample_range 2S | memory_idx S | hand_idx S] int64, [slot_seen S] int32, [use_memory S] bytes
  const size_t nf = (size_t)2 * S * 25 + 132 + (size_t)S * (648 + 16 + 60 + 64);
  const size_t off_i64 = (nf * 4 + 7) / 8 * 8, off_i32 = off_i64 + (size_t)4 * S * 8, off_u8 = off_i32 + (size_t)S * 4, total = off_u8 + S;
  std::vector<char> host(total, 0);
  float* f = reinterpret_cast<float*>(host.data());
  for (int c = 0; c < 2 * S; ++c) {
    float* k = f + (size_t)c * 9;
    k[0] = k[4] = 130.f; k[2] = k[5] = 47.5f; k[8] = 1.f;
    float* x = f + (size_t)2 * S * 9 + (size_t)c * 16;
    x[0] = x[5] = x[10] = x[15] = 1.f;
    if (c & 1) x[3] = 0.06f;
  }
  long long* i64 = reinterpret_cast<long long*>(host.data() + off_i64);
  for (int k = 0; k < S; ++k) { i64[2 * k] = 2 * k; i64[2 * k + 1] = 2 * k + 2; i64[2 * S + k] = k; i64[3 * S + k] = k & 1; }
  void* dv = nullptr;
  HIPCHK(h, hipMalloc(&dv, total));
  hipError_t e = hipMemcpyAsync(dv, host.data(), total, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { (void)hipFree(dv); return fail(h, UT_E_HIP, "calibration descriptors", e); }
  char* d = static_cast<char*>(dv);
  float* df = reinterpret_cast<float*>(d);
  ut::HeadArgs a{};
  a.feat = feat; a.intrinsics = df; a.extrinsics = df + (size_t)2 * S * 9;
  const float* skel = df + (size_t)2 * S * 25;
  a.mem = df + (size_t)2 * S * 25 + 132; a.prev_ext = a.mem + (size_t)S * 648;
  float* pose = a.prev_ext + (size_t)S * 16;
  float* raw = pose + (size_t)S * 60;
  a.sample_range = reinterpret_cast<const int64_t*>(d + off_i64); a.memory_idx = a.sample_range + 2 * S; a.hand_idx = a.memory_idx + S;
  a.slot_seen = reinterpret_cast<int*>(d + off_i32); a.use_memory = reinterpret_cast<const uint8_t*>(d + off_u8);
  a.n_samples = S; a.n_crops = 2 * S; a.n_slots = S; a.status = h->status; a.call_error_mask = 0;
  rc = begin_call(h, s);
  for (int mode = 0; mode < 2 && !rc; ++mode) rc = run_head(h, a, skel, 1, mode == 0 ? UT_MODE_KNOWN_SKELETON : UT_MODE_UNKNOWN_SKELETON, pose, raw, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(dv);
  return rc;
}

// Calibration of the split-fp16 activation scales: `crops` (device fp32 [n,96,96]) through the backbone with the per-launch
// (dynamic) scales, every tensor's largest magnitude folded into its calibrated word, then raised by 2^kCalibHeadroom.
// Synchronous; the status words are left as they were (a calibration pass reports nothing: a non-finite activation ends up in
// the calibrated word and is flagged by the calls that use it).
static int calibrate_split(ut_handle h, const float* crops, int n, hipStream_t s) {
  // The modes a calibration pass pins, put back on every way out.  Latency mode among them: it keeps every launch on the
  // fp32 instruction without a max word, which would leave all the words at zero.
  struct PinnedModes {
    ut_handle h;
    const int conv_arith, lanes;
    const bool profiling, block_fusion, latency_mode;
    explicit PinnedModes(ut_handle hh)
        : h(hh), conv_arith(hh->conv_arith), lanes(hh->lanes), profiling(hh->profiling), block_fusion(hh->block_fusion),
          latency_mode(hh->latency_mode) {
      h->conv_arith = UT_CONV_SPLIT_F16_ALWAYS; h->lanes = 1; h->profiling = false; h->latency_mode = false; h->calibrating = true;
    }
    ~PinnedModes() {
      h->conv_arith = conv_arith; h->lanes = lanes; h->profiling = profiling; h->block_fusion = block_fusion;
      h->latency_mode = latency_mode; h->calibrating = false;
    }
  };
  float* feat = nullptr;
  int rc = dev_alloc(h, &feat, (size_t)n * 72 * 36);
  if (rc) return rc;
  rc = [&]() -> int {
    PinnedModes pinned(h);
    int saved[2] = {0, 0}, r;
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipMemcpy(saved, h->status, sizeof saved, hipMemcpyDeviceToHost));
    h->calibrated = h->head_calibrated = false;      // until the words are whole again
    HIPCHK(h, ut::launch_zero_words(h->calib, 64, s));
    // both launch forms of layer1 / layer2's entry: the separate-launch form (ut_set_block_fusion(h, 0)) has two tensors more
    for (int form = 0; form < 2; ++form) {
      h->block_fusion = form == 0;
      if ((r = run_backbone(h, crops, nullptr, n, feat, s))) return r;
    }
    const bool with_head = n >= 2;
    if (with_head && (r = calibrate_head(h, feat, n, s))) return r;
    HIPCHK(h, ut::launch_raise_words(h->calib, kScaleTensors, kCalibHeadroom, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipMemcpy(h->status, saved, sizeof saved, hipMemcpyHostToDevice));
    h->calibrated = true;
    h->head_calibrated = with_head;
    return UT_OK;
  }();
  (void)hipStreamSynchronize(s);
  dev_free(h, feat);
  return rc;
}

constexpr int kBuiltinCalibCrops = 64;

static int calibrate_builtin(ut_handle h) {
  float* crops = nullptr;
  int rc = dev_alloc(h, &crops, (size_t)kBuiltinCalibCrops * 96 * 96);
  if (rc) return rc;
  hipError_t e = ut::launch_calibration_crops(crops, kBuiltinCalibCrops, 0);
  rc = e != hipSuccess ? fail(h, UT_E_HIP, "launch_calibration_crops", e) : calibrate_split(h, crops, kBuiltinCalibCrops, 0);
  (void)hipDeviceSynchronize();
  dev_free(h, crops);
  return rc;
}

int ut_calibrate_split(ut_handle h, const float* crops, int n_crops, void* stream) {
  if (!h) return UT_E_INVALID;
  if (n_crops < 0 || (n_crops > 0 && !crops)) return fail(h, UT_E_INVALID, "ut_calibrate_split: bad argument");
  ON_DEVICE_OF(h);
  return n_crops == 0 ? calibrate_builtin(h) : calibrate_split(h, crops, n_crops, (hipStream_t)stream);
}

int ut_set_split_scale(ut_handle h, int mode) {
  if (!h || (mode != UT_SPLIT_SCALE_CALIBRATED && mode != UT_SPLIT_SCALE_DYNAMIC && mode != UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE))
    return fail(h, UT_E_INVALID, "ut_set_split_scale: bad argument");
  ON_DEVICE_OF(h);
  h->scale_mode = mode;
  if (mode != UT_SPLIT_SCALE_DYNAMIC && h->conv_arith != UT_CONV_FP32 && !h->calibrated) return calibrate_builtin(h);
  return UT_OK;
}

int ut_get_split_adaptations(ut_handle h, uint32_t* out, int reset, void* stream) {
  if (!h || !out) return fail(h, UT_E_INVALID, "ut_get_split_adaptations: null argument");
  ON_DEVICE_OF(h);
  hipStream_t s = (hipStream_t)stream;
  unsigned n = 0;
  HIPCHK(h, hipMemcpyAsync(&n, h->adapt_count, sizeof n, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  *out = n;
  if (reset) {
    HIPCHK(h, ut::launch_zero_words(h->adapt_count, 1, s));      // a kernel, not a memset node: see launch_zero_words
    HIPCHK(h, hipStreamSynchronize(s));
  }
  return UT_OK;
}

int ut_get_split_calibration(ut_handle h, float* out33) {
  if (!h || !out33) return fail(h, UT_E_INVALID, "ut_get_split_calibration: null argument");
  ON_DEVICE_OF(h);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out33, h->calib, kScaleTensors * sizeof(float), hipMemcpyDeviceToHost));
  return h->calibrated ? UT_OK : 1;
}

int ut_backbone(ut_handle h, const float* crops, int n_crops, float* feat, void* stream) {
  if (!h) return UT_E_INVALID;
  if (n_crops == 0) return UT_OK;
  if (!crops || !feat || n_crops < 0) return fail(h, UT_E_INVALID, "ut_backbone: bad argument");
  ON_DEVICE_OF(h);
  return run_backbone(h, crops, nullptr, n_crops, feat, (hipStream_t)stream);
}

int ut_warp_backbone(ut_handle h, const uint8_t* src, int n_src_images, int src_h, int src_w, const double* cam_params,
                     const double* crop_params, const int32_t* src_index, int n_crops, int remap_mode, float* feat,
                     void* stream) {
  if (!h) return UT_E_INVALID;
  if (n_crops == 0) return UT_OK;
  if (!src || !cam_params || !crop_params || !src_index || !feat || n_crops < 0 || src_h <= 0 || src_w <= 0 ||
      n_src_images <= 0 || (remap_mode != UT_REMAP_CV2_FIXED && remap_mode != UT_REMAP_FLOAT))
    return fail(h, UT_E_INVALID, "ut_warp_backbone: bad argument");
  ON_DEVICE_OF(h);
  hipStream_t s = (hipStream_t)stream;
  const bool u8 = remap_mode == UT_REMAP_CV2_FIXED;
  int rc = regrow(h, &h->crops_ws_floats, (size_t)n_crops * 96 * 96 / (u8 ? sizeof(float) : 1), {{&h->crops_ws, 1}});
  if (rc) return rc;
  HIPCHK(h, ut::launch_warp(src, n_src_images, src_h, src_w, cam_params, crop_params, src_index, n_crops, remap_mode,
                            u8 ? nullptr : h->crops_ws, u8 ? (uint8_t*)h->crops_ws : nullptr, h->status, s));
  if (h->check_mode == UT_CHECK_SYNC && (rc = check_status(h, h->status, h->status_host, s, "ut_warp_backbone"))) return rc;
  return run_backbone(h, u8 ? nullptr : h->crops_ws, u8 ? (const uint8_t*)h->crops_ws : nullptr, n_crops, feat, s);
}

// The head behind the index checks: FTL, fusion, temporal block, regressor, decode (a.mem / a.prev_ext: the temporal state it
// reads and writes - the handle's, or scratch during a calibration pass).
// The regressor's four 3x3 convolutions (76 or 72 channels on the 6x6 map: 80 % of the head's arithmetic) run in the split-fp16
// arithmetic when the call is large enough to fill the chip with conv_w4's tiles: their tensors are then laid out with 128
// channels (zeros behind the real ones; zero weight rows and columns), the shape of layer3 at a 6x6 map.
static int run_head(ut_handle h, const ut::HeadArgs& a, const float* skel, int n_skel, int mode, float* out_pose, float* out_raw,
                    hipStream_t s) {
  int rc;
  const ut::HeadBuffers& b = h->hb;
  const int S = a.n_samples;
  h->call_split = false;             // fusion and temporal block: 1x1 convolutions, on the fp32 matrix instruction
  HIPCHK(h, ut::launch_ftl_in(a, b, h->block_fusion, s));
  // fusion and temporal chain: one streaming launch each, which leaves the intermediates of the layer-by-layer form (f108 and
  // f72a; t92b and t92a in turn) unwritten
  bool chained = false;
  if ((rc = run_pw(h, {&h->fus0, &h->fus1, &h->fus2}, {true, true, false}, b.cat144, b.f72b, S, 6, 6, false, s, &chained))) return rc;
  if (!chained) {
    if ((rc = run_conv(h, h->fus0, b.cat144, nullptr, b.f108, S, 6, 6, true, false, s))) return rc;
    if ((rc = run_conv(h, h->fus1, b.f108, nullptr, b.f72a, S, 6, 6, true, false, s))) return rc;
    if ((rc = run_conv(h, h->fus2, b.f72a, nullptr, b.f72b, S, 6, 6, false, false, s))) return rc;
  }
  HIPCHK(h, ut::launch_ftl_out_temporal_in(a, b, s));
  if ((rc = run_pw(h, {&h->tmp[0], &h->tmp[1], &h->tmp[2]}, {true, true, false}, b.t92a, b.t92b, S, 6, 6, false, s, &chained))) return rc;
  if (!chained) {
    if ((rc = run_conv(h, h->tmp[0], b.t92a, nullptr, b.t92b, S, 6, 6, true, false, s))) return rc;
    if ((rc = run_conv(h, h->tmp[1], b.t92b, nullptr, b.t92a, S, 6, 6, true, false, s))) return rc;
    if ((rc = run_conv(h, h->tmp[2], b.t92a, nullptr, b.t92b, S, 6, 6, false, false, s))) return rc;
  }
  const Regressor& reg = mode == UT_MODE_KNOWN_SKELETON ? h->reg_k : h->reg_u;
  if (mode == UT_MODE_KNOWN_SKELETON)
    HIPCHK(h, ut::launch_skeleton(skel, h->skel_w, h->skel_b, h->skel_scale, h->skel_shift, b.skel, n_skel, s));
  // split-fp16 regressor: chosen per call like the backbone's arithmetic (UT_CONV_SPLIT_F16: from 4 x CUs samples = one tile of
  // 8 samples per CU and wave set), with calibrated scales only once the head has been calibrated
  const bool head_split = !h->latency_mode && (h->calibrating || h->scale_mode == UT_SPLIT_SCALE_DYNAMIC || h->head_calibrated) &&
                          (h->conv_arith == UT_CONV_SPLIT_F16_ALWAYS || (h->conv_arith == UT_CONV_SPLIT_F16 && S >= 4 * h->num_cu));
  const int stride = head_split ? ut::kRegSplitCh : reg.c;
  const int tid0 = mode == UT_MODE_KNOWN_SKELETON ? 25 : 29;
  unsigned* in_word = nullptr;
  if (head_split) {
    if ((rc = lease_words(h, s, 16))) return rc;
    in_word = h->counters + kMaxCounters + take_word(h);
  }
  HIPCHK(h, ut::launch_temporal_out(a, b.t92b, b.skel, n_skel, b.regin, reg.c, stride, in_word, s));
  // two BasicBlocks on the 6x6 map (lib/models/model_utils.py:195-208)
  h->call_split = head_split;
  const Block* blocks = head_split ? reg.blocks_split : reg.blocks;
  unsigned* mid_word = nullptr;
  rc = run_block(h, blocks[0], b.regin, b.rega, nullptr, b.regb, S, 6, 6, s, in_word, &mid_word, head_split ? tid0 : -1, head_split ? tid0 + 1 : -1);
  if (!rc) rc = run_block(h, blocks[1], b.regb, b.rega, nullptr, b.regin, S, 6, 6, s, mid_word, nullptr, head_split ? tid0 + 2 : -1, head_split ? tid0 + 3 : -1);
  h->call_split = false;
  if (!rc) rc = flush_chain(h);      // the regressor's chain
  if (rc) { h->chain.clear(); h->chain_flops = 0; return rc; }
  HIPCHK(h, ut::launch_pool_decode(a, b.regin, reg.c, stride, reg.w_out, reg.b_out, reg.d, out_pose, out_raw, b.rega, s));
  return UT_OK;
}

int ut_fuse_temporal_regress(ut_handle h, const float* feat, const float* intrinsics, const float* extrinsics,
                             const int64_t* sample_range, const int64_t* memory_idx, const uint8_t* use_memory,
                             const int64_t* hand_idx, int n_crops, int n_samples, int n_slots, int all_multiview,
                             const float* skel, int n_skel, int mode, float* out_pose, float* out_raw, void* stream) {
  if (!h) return UT_E_INVALID;
  if (n_samples == 0) return UT_OK;
  if (!feat || !intrinsics || !extrinsics || !sample_range || !memory_idx || !use_memory || !hand_idx || !out_pose ||
      n_samples < 0 || n_crops < n_samples || n_crops > 2 * n_samples || n_slots <= 0)
    return fail(h, UT_E_INVALID, "ut_fuse_temporal_regress: bad argument");
  if (mode == UT_MODE_KNOWN_SKELETON) {
    if (!skel || (n_skel != 1 && n_skel != n_samples))
      return fail(h, UT_E_INVALID, "ut_fuse_temporal_regress: skeleton must have 1 or n_samples entries");
  } else if (mode == UT_MODE_UNKNOWN_SKELETON) {
    // lib/models/umetrack_model.py:224-229
    if (!all_multiview)
      return fail(h, UT_E_UNSUPPORTED, "Unsupported: found single-view samples when calibration scale");
    n_skel = 0;
  } else {
    return fail(h, UT_E_INVALID, "ut_fuse_temporal_regress: unknown mode");
  }
  ON_DEVICE_OF(h);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = ensure_head_ws(h, n_samples, n_skel))) return rc;
  if ((rc = ensure_slots(h, n_slots, s))) return rc;
  if ((rc = begin_call(h, s))) return rc;
  h->call_split = false;             // the head stays on the fp32 matrix instructions
  ut::HeadArgs a{};
  a.feat = feat; a.intrinsics = intrinsics; a.extrinsics = extrinsics; a.sample_range = sample_range;
  a.memory_idx = memory_idx; a.use_memory = use_memory; a.hand_idx = hand_idx; a.n_samples = n_samples;
  a.n_crops = n_crops; a.n_slots = n_slots;
  a.mem = h->mem; a.prev_ext = h->prev_ext;
  a.status = h->status; a.slot_seen = h->slot_seen;
  a.call_error_mask = mode == UT_MODE_UNKNOWN_SKELETON ? ut::UT_SINGLE_VIEW : 0;
  // index checks (stream ordered, in front of everything that indexes with the descriptors)
  HIPCHK(h, ut::launch_zero_words(h->status + 1, 1, s));
  HIPCHK(h, ut::launch_zero_words(h->slot_seen, (size_t)n_slots, s));
  HIPCHK(h, ut::launch_validate_desc(a, s));
  if (h->check_mode == UT_CHECK_SYNC) {
    if ((rc = check_status(h, h->status, h->status_host, s, "ut_fuse_temporal_regress"))) return rc;
    if (h->status_host[1] & a.call_error_mask)   // lib/models/umetrack_model.py:224-229
      return fail(h, UT_E_UNSUPPORTED, "Unsupported: found single-view samples when calibration scale");
  }
  if (n_slots > h->slots_used) h->slots_used = n_slots;
  return run_head(h, a, skel, n_skel, mode, out_pose, out_raw, s);
}

int ut_reset_memory(ut_handle h) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  HIPCHK(h, hipDeviceSynchronize());
  if (h->slots_cap) {
    HIPCHK(h, hipMemset(h->mem, 0, (size_t)h->slots_cap * 36 * 18 * sizeof(float)));
    HIPCHK(h, hipMemset(h->prev_ext, 0, (size_t)h->slots_cap * 16 * sizeof(float)));
  }
  h->slots_used = 0;
  return UT_OK;
}

int ut_get_memory(ut_handle h, float* mem, float* prev_ext, int max_slots, void* stream) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  int n = h->slots_used < max_slots ? h->slots_used : max_slots;
  if (n > 0) {
    if (!mem || !prev_ext) return fail(h, UT_E_INVALID, "ut_get_memory: null output");
    HIPCHK(h, ut::launch_mem_export(h->mem, mem, n, (hipStream_t)stream));
    HIPCHK(h, hipMemcpyAsync(prev_ext, h->prev_ext, (size_t)n * 16 * sizeof(float), hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
  }
  return h->slots_used;
}

int ut_fk(ut_handle h, const float* hand_model, int n_models, const float* joint_angles, int ja_stride,
          const float* wrist_xf, int xf_stride, const int64_t* mirror, float t_scale, int n, float* out, void* stream) {
  // stateless: h may be NULL (errors then land in the thread-local slot read by ut_last_error(NULL))
  if (n == 0) return UT_OK;
  if (!hand_model || !joint_angles || !wrist_xf || !out || n < 0 || (n_models != 1 && n_models != n) ||
      ja_stride < 22 || xf_stride < 16)
    return fail(h, UT_E_INVALID, "ut_fk: bad argument");
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_fk(hand_model, n_models, joint_angles, ja_stride, wrist_xf, xf_stride, mirror, t_scale, n, out,
                          (hipStream_t)stream));
  return UT_OK;
}

namespace {
int fail_as(ut_handle h, const char* who, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fail(h, UT_E_INVALID, msg);
}

// The argument checks the pose fits share, on the arguments as the kernels get them; `who` names the entry in the message.
// FIT_NO_TARGETS: the fits in the views, which have no 3-D targets and need their start.  FIT_POSE_IS_INPUT: ut_pose_information_views,
// whose pose stands where the fits have their start - it is checked as their outputs are; a.ja / a.xf and a.max_iters are not read.
// FIT_START_OPTIONAL: ut_track_pose_views, whose sequences may start from the cold rows instead - the entry checks that one of them is there.
enum : int { FIT_NO_TARGETS = 1, FIT_POSE_IS_INPUT = 2, FIT_START_OPTIONAL = 4 };
int fit_pose_args(ut_handle h, const char* who, const ut::FitPoseArgs& a, int flags = 0) {
  const bool with_targets = !(flags & FIT_NO_TARGETS), fitted = !(flags & FIT_POSE_IS_INPUT);
  const float *ja = fitted ? a.ja : a.init_ja, *xf = fitted ? a.xf : a.init_xf;
  const int ja_stride = fitted ? a.ja_stride : a.init_ja_stride, xf_stride = fitted ? a.xf_stride : a.init_xf_stride;
  if (!a.hand_model || (with_targets && !a.targets) || !ja || !xf || a.n < 0 || (a.n_models != 1 && a.n_models != a.n))
    return fail_as(h, who, "bad argument");
  if (!with_targets && !(flags & FIT_START_OPTIONAL) && (!a.init_ja || !a.init_xf))
    return fail_as(h, who, "init_angles and init_wrist_xf are required: there is no cold start");
  if ((a.init_ja == nullptr) != (a.init_xf == nullptr))
    return fail_as(h, who, "init_angles and init_wrist_xf must both be given or both be NULL");
  if ((with_targets && a.target_stride < 63) || ja_stride < 22 || xf_stride < 12 ||
      (a.init_ja && (a.init_ja_stride < 22 || a.init_xf_stride < 12)))
    return fail_as(h, who, "a stride is below 63 (targets) / 22 (angles) / 12 (wrist)");
  if (fitted && (a.max_iters < 1 || a.max_iters > 256)) return fail_as(h, who, "max_iters must be in 1..256");
  if (!(a.t_scale > 0.f) || !(a.t_scale <= 3.0e38f)) return fail_as(h, who, "t_scale must be positive and finite");
  return UT_OK;
}
}  // namespace

int ut_fit_pose(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                const float* weights, const float* limits, const float* init_angles, int init_ja_stride,
                const float* init_wrist_xf, int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int n,
                float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream) {
  // stateless like ut_fk: h may be NULL
  if (n == 0) return UT_OK;
  const ut::FitArgs a{{hand_model, n_models, targets, target_stride, limits, init_angles, init_ja_stride, init_wrist_xf,
                       init_xf_stride, mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                      weights, info};
  const int rc = fit_pose_args(h, "ut_fit_pose", a.pose);
  if (rc) return rc;
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_fit_pose(a, (hipStream_t)stream));
  return UT_OK;
}

int ut_fit_pose_info(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                     const float* sqrt_info, const float* limits, const float* init_angles, int init_ja_stride,
                     const float* init_wrist_xf, int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int n,
                     float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream) {
  // stateless like ut_fit_pose: h may be NULL
  if (n == 0) return UT_OK;
  if (!sqrt_info) return fail(h, UT_E_INVALID, "ut_fit_pose_info: bad argument");
  const ut::FitInfoArgs a{{hand_model, n_models, targets, target_stride, limits, init_angles, init_ja_stride, init_wrist_xf,
                           init_xf_stride, mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                          sqrt_info, info};
  const int rc = fit_pose_args(h, "ut_fit_pose_info", a.pose);
  if (rc) return rc;
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_fit_pose_info(a, (hipStream_t)stream));
  return UT_OK;
}

static_assert(UT_SCALE_FREE == ut::FITS_MODE_FREE && UT_SCALE_FIXED == ut::FITS_MODE_FIXED && UT_SCALE_MIN == ut::FITS_SCALE_MIN &&
              UT_SCALE_MAX == ut::FITS_SCALE_MAX && UT_SCALE_INFO_LAMBDA == ut::FITS_SCALE_INFO_LAMBDA &&
              UT_FITS_CONVERGED == ut::FITS_CONVERGED && UT_FITS_AT_MAX_ITERS == ut::FITS_AT_MAX_ITERS &&
              UT_FITS_REFUSED == ut::FITS_REFUSED && UT_FITS_AT_BOUND == ut::FITS_AT_BOUND, "umetrack_hip_scale.h and ut_kernels.h");

int ut_fit_pose_scale(ut_handle h, const float* hand_model, int n_models, const float* targets, int target_stride,
                      const float* weights, const float* limits, const float* init_scale, int scale_mode,
                      const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                      const int64_t* mirror, float t_scale, int max_iters, int n, float* joint_angles, int ja_stride,
                      float* wrist_xf, int xf_stride, float* scale, float* info, void* stream) {
  // stateless like ut_fit_pose: h may be NULL
  if (n == 0) return UT_OK;
  if (!scale) return fail(h, UT_E_INVALID, "ut_fit_pose_scale: bad argument");
  if (scale_mode != UT_SCALE_FREE && scale_mode != UT_SCALE_FIXED)
    return fail(h, UT_E_INVALID, "ut_fit_pose_scale: scale_mode must be UT_SCALE_FREE or UT_SCALE_FIXED");
  const ut::FitScaleArgs a{{hand_model, n_models, targets, target_stride, limits, init_angles, init_ja_stride, init_wrist_xf,
                            init_xf_stride, mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                           weights, init_scale, scale_mode, scale, info};
  const int rc = fit_pose_args(h, "ut_fit_pose_scale", a.pose);
  if (rc) return rc;
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_fit_pose_scale(a, (hipStream_t)stream));
  return UT_OK;
}

int ut_pool_scale(ut_handle h, const float* scale, const float* info, int n_groups, int group_size, float* group,
                  float* pose_scale, void* stream) {
  if (n_groups == 0) return UT_OK;
  if (!scale || !info || !group || n_groups < 0 || group_size < 1) return fail(h, UT_E_INVALID, "ut_pool_scale: bad argument");
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_pool_scale(scale, info, n_groups, group_size, group, pose_scale, (hipStream_t)stream));
  return UT_OK;
}

struct ut_mesh {
  int device = 0;
  int n_vertices = 0, n_triangles = 0;
  void* verts = nullptr;          // float4 [n_vertices][2], see launch_skin_mesh
  uint32_t* csr_off = nullptr;    // [n_vertices + 1]
  uint32_t* csr_ent = nullptr;    // [3 * n_triangles]
  int32_t* tris = nullptr;        // int4 [n_triangles]: (a, b, c, 0), the list ut_render_mesh walks
};
static_assert(UT_MESH_MAX_VERTICES == ut::MESH_MAX_VERTICES && UT_MESH_MAX_VERTICES <= 65536, "vertex cap");

int ut_mesh_create(const float* vertices, int n_vertices, const int32_t* triangles, int n_triangles,
                   const float* dense_bone_weights, int device, ut_mesh** out) {
  if (out) *out = nullptr;
  if (!out || !vertices || !dense_bone_weights || (!triangles && n_triangles != 0))
    return fail(nullptr, UT_E_INVALID, "ut_mesh_create: null argument");
  if (n_vertices <= 0) return fail(nullptr, UT_E_INVALID, "ut_mesh_create: the mesh has no vertices");
  if (n_triangles < 0) return fail(nullptr, UT_E_INVALID, "ut_mesh_create: negative triangle count");
  char msg[256];
  if (n_vertices > UT_MESH_MAX_VERTICES) {
    snprintf(msg, sizeof msg, "ut_mesh_create: %d vertices, more than UT_MESH_MAX_VERTICES (%d) that fit a workgroup's LDS",
             n_vertices, UT_MESH_MAX_VERTICES);
    return fail(nullptr, UT_E_UNSUPPORTED, msg);
  }
  if (n_triangles > (1 << 24)) return fail(nullptr, UT_E_UNSUPPORTED, "ut_mesh_create: more than 2^24 triangles");
  // ---- pack on the host: (x, y, z, bones) | weights per vertex, slots in ascending bone order
  const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles;
  std::vector<float> packed(nv * 8, 0.f);
  for (size_t v = 0; v < nv; ++v) {
    float* p = &packed[v * 8];
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(vertices[3 * v + k])) {
        snprintf(msg, sizeof msg, "ut_mesh_create: vertex %zu has a coordinate that is not finite", v);
        return fail(nullptr, UT_E_INVALID, msg);
      }
      p[k] = vertices[3 * v + k];
    }
    uint32_t bones = 0;
    int slots = 0;
    for (int f = 0; f < 17; ++f) {
      const float w = dense_bone_weights[17 * v + f];
      if (!std::isfinite(w)) {
        snprintf(msg, sizeof msg, "ut_mesh_create: weight [%zu][%d] is not finite", v, f);
        return fail(nullptr, UT_E_INVALID, msg);
      }
      if (w == 0.f) continue;
      if (slots == UT_MESH_MAX_INFLUENCES) {
        snprintf(msg, sizeof msg, "ut_mesh_create: vertex %zu has more than %d non-zero bone weights", v,
                 UT_MESH_MAX_INFLUENCES);
        return fail(nullptr, UT_E_UNSUPPORTED, msg);
      }
      bones |= (uint32_t)f << (8 * slots);
      p[4 + slots] = w;
      ++slots;
    }
    memcpy(&p[3], &bones, sizeof bones);
  }
  // ---- vertex -> incident triangles, ascending triangle order, each entry rotated so that the vertex comes first
  std::vector<uint32_t> off(nv + 1, 0), ent(nt * 3 + 1, 0);
  for (size_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) {
      const int32_t v = triangles[3 * t + k];
      if (v < 0 || v >= n_vertices) {
        snprintf(msg, sizeof msg, "ut_mesh_create: triangle %zu names vertex %d, outside [0, %d)", t, (int)v, n_vertices);
        return fail(nullptr, UT_E_INVALID, msg);
      }
      ++off[(size_t)v + 1];
    }
  for (size_t v = 0; v < nv; ++v) off[v + 1] += off[v];
  {
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (size_t t = 0; t < nt; ++t)
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = (uint32_t)triangles[3 * t + k];
        const uint32_t a = (uint32_t)triangles[3 * t + (k + 1) % 3], b = (uint32_t)triangles[3 * t + (k + 2) % 3];
        ent[fill[v]++] = a | (b << 16);
      }
  }
  std::vector<int32_t> tri4(nt * 4 + 4, 0);
  for (size_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) tri4[4 * t + k] = triangles[3 * t + k];
  // ---- upload
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return fail(nullptr, UT_E_HIP, "hipSetDevice", scope.err);
  ut_mesh* m = new ut_mesh();
  m->device = device; m->n_vertices = n_vertices; m->n_triangles = n_triangles;
  hipError_t e = hipMalloc(&m->verts, packed.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&m->csr_off, off.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m->csr_ent, ent.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m->tris, tri4.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(m->tris, tri4.data(), tri4.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->verts, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->csr_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->csr_ent, ent.data(), ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(m->verts); (void)hipFree(m->csr_off); (void)hipFree(m->csr_ent); (void)hipFree(m->tris);
    delete m;
    return fail(nullptr, UT_E_HIP, "ut_mesh_create: upload", e);
  }
  *out = m;
  return UT_OK;
}

int ut_mesh_destroy(ut_mesh* m) {
  if (!m) return UT_OK;
  DeviceScope scope(m->device);
  (void)hipFree(m->verts); (void)hipFree(m->csr_off); (void)hipFree(m->csr_ent); (void)hipFree(m->tris);
  delete m;
  return UT_OK;
}

int ut_mesh_counts(const ut_mesh* m, int* n_vertices, int* n_triangles) {
  if (!m) return fail(nullptr, UT_E_INVALID, "ut_mesh_counts: null mesh");
  if (n_vertices) *n_vertices = m->n_vertices;
  if (n_triangles) *n_triangles = m->n_triangles;
  return UT_OK;
}

int ut_skin_mesh(ut_handle h, const ut_mesh* mesh, const float* hand_model, int n_models, const float* joint_angles,
                 int ja_stride, const float* wrist_xf, int xf_stride, const int64_t* mirror, float t_scale, int n,
                 float* out_vertices, float* out_normals, void* stream) {
  if (!mesh) return fail(h, UT_E_INVALID, "ut_skin_mesh: null mesh");
  if (h && h->device != mesh->device) return fail(h, UT_E_INVALID, "ut_skin_mesh: the mesh lives on another device than the handle");
  if (n == 0) return UT_OK;
  if (!hand_model || !joint_angles || !wrist_xf || !out_vertices || n < 0 || (n_models != 1 && n_models != n) ||
      ja_stride < 22 || xf_stride < 16)
    return fail(h, UT_E_INVALID, "ut_skin_mesh: bad argument");
  DeviceScope scope(mesh->device);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  HIPCHK(h, ut::launch_skin_mesh(hand_model, n_models, joint_angles, ja_stride, wrist_xf, xf_stride, mirror, t_scale, n,
                                 mesh->verts, mesh->csr_off, mesh->csr_ent, mesh->n_vertices, out_vertices, out_normals,
                                 (hipStream_t)stream));
  return UT_OK;
}

namespace {
// the status words an entry with an optional handle checks into, and whether it reads them back itself
struct StatusTarget { int *dev = nullptr, *host = nullptr, mode = UT_CHECK_SYNC, device = 0; };
int status_target(ut_handle h, StatusTarget* t) {
  if (h) { t->dev = h->status; t->host = h->status_host; t->mode = h->check_mode; t->device = h->device; return UT_OK; }
  DevStatus st;
  int rc = stateless_status(&t->device, &st);
  if (rc) return rc;
  t->dev = st.dev; t->host = st.host;
  return UT_OK;
}
}  // namespace

int ut_project_points(ut_handle h, const float* points, int point_stride, int n_points, const int32_t* cam_rows,
                      int max_views, const double* table, int n_rows, int table_kind, int n, int width, int height,
                      double* window, double* eye_z, uint8_t* flags, void* stream) {
  if (!points || !cam_rows || !table || !window || !eye_z || !flags)
    return fail(h, UT_E_INVALID, "ut_project_points: null argument");
  if (table_kind != UT_CAMERA_FISHEYE62 && table_kind != UT_CAMERA_PINHOLE)
    return fail(h, UT_E_INVALID, "ut_project_points: table_kind must be UT_CAMERA_FISHEYE62 or UT_CAMERA_PINHOLE");
  if (n < 0 || n_points <= 0 || max_views <= 0 || n_rows <= 0 || point_stride < 3 * n_points || width < 0 || height < 0)
    return fail(h, UT_E_INVALID, "ut_project_points: bad argument");
  if (n == 0) return UT_OK;
  StatusTarget st;
  int rc = status_target(h, &st);
  if (rc) return rc;
  DeviceScope scope(st.device);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  hipStream_t s = (hipStream_t)stream;
  ut::ProjectArgs g{};
  g.points = points; g.point_stride = point_stride; g.n_points = n_points; g.cam_rows = cam_rows; g.max_views = max_views;
  g.table = table; g.n_rows = n_rows; g.kind = table_kind == UT_CAMERA_FISHEYE62 ? ut::PROJECT_FISHEYE62 : ut::PROJECT_PINHOLE;
  g.n = n; g.width = width; g.height = height; g.window = window; g.eye_z = eye_z; g.flags = flags; g.status = st.dev;
  HIPCHK(h, ut::launch_project_points(g, s));
  return st.mode == UT_CHECK_SYNC ? check_status(h, st.dev, st.host, s, "ut_project_points") : UT_OK;
}

static_assert(UT_TRI_MAX_VIEWS == ut::TRI_MAX_VIEWS && UT_TRI_CONVERGED == ut::TRI_CONVERGED && UT_TRI_AT_MAX_ITERS == ut::TRI_AT_MAX_ITERS &&
              UT_TRI_REFUSED == ut::TRI_REFUSED && UT_TRI_DEGENERATE == ut::TRI_DEGENERATE, "triangulation constants");

namespace {
// ut_triangulate_points and ut_triangulate_points_info: one path, sqrt_info null for the former; `who` names the entry.
int triangulate_points(ut_handle h, const char* who, const double* window, const float* weights, const int32_t* cam_rows,
                       int max_views, const double* table, int n_rows, int table_kind, int n_points, int n, int max_iters,
                       double* points, float* points_f32, int point_stride, float* info, float* residual, float* sqrt_info,
                       void* stream) {
  if (!window || !cam_rows || !table) return fail_as(h, who, "null argument");
  if (!points && !points_f32) return fail_as(h, who, "one of points and points_f32 must be given");
  if (table_kind != UT_CAMERA_FISHEYE62 && table_kind != UT_CAMERA_PINHOLE)
    return fail_as(h, who, "table_kind must be UT_CAMERA_FISHEYE62 or UT_CAMERA_PINHOLE");
  if (max_views < 1 || max_views > UT_TRI_MAX_VIEWS) return fail_as(h, who, "max_views must be in 1..UT_TRI_MAX_VIEWS (8)");
  if (max_iters < 1 || max_iters > 64) return fail_as(h, who, "max_iters must be in 1..64");
  if (n < 0 || n_points < 1 || n_rows < 1 || (points_f32 && point_stride < 3 * n_points)) return fail_as(h, who, "bad argument");
  if (n == 0) return UT_OK;
  if (h) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, window) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device != h->device)
      return fail_as(h, who, "the windows live on another device than the handle");
  }
  StatusTarget st;
  int rc = status_target(h, &st);
  if (rc) return rc;
  DeviceScope scope(st.device);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  hipStream_t s = (hipStream_t)stream;
  ut::TriArgs g{};
  g.window = window; g.weights = weights; g.cam_rows = cam_rows; g.max_views = max_views; g.table = table; g.n_rows = n_rows;
  g.kind = table_kind == UT_CAMERA_FISHEYE62 ? ut::PROJECT_FISHEYE62 : ut::PROJECT_PINHOLE;
  g.n_points = n_points; g.n = n; g.max_iters = max_iters; g.points = points; g.points_f32 = points_f32;
  g.point_stride = point_stride; g.info = info; g.residual = residual; g.status = st.dev; g.sqrt_info = sqrt_info;
  HIPCHK(h, ut::launch_triangulate(g, s));
  return st.mode == UT_CHECK_SYNC ? check_status(h, st.dev, st.host, s, who) : UT_OK;
}
}  // namespace

int ut_triangulate_points(ut_handle h, const double* window, const float* weights, const int32_t* cam_rows, int max_views,
                          const double* table, int n_rows, int table_kind, int n_points, int n, int max_iters,
                          double* points, float* points_f32, int point_stride, float* info, float* residual, void* stream) {
  return triangulate_points(h, "ut_triangulate_points", window, weights, cam_rows, max_views, table, n_rows, table_kind, n_points,
                            n, max_iters, points, points_f32, point_stride, info, residual, nullptr, stream);
}

int ut_triangulate_points_info(ut_handle h, const double* window, const float* weights, const int32_t* cam_rows, int max_views,
                               const double* table, int n_rows, int table_kind, int n_points, int n, int max_iters,
                               double* points, float* points_f32, int point_stride, float* info, float* residual,
                               float* sqrt_info, void* stream) {
  if (!sqrt_info) return fail(h, UT_E_INVALID, "ut_triangulate_points_info: null argument");
  return triangulate_points(h, "ut_triangulate_points_info", window, weights, cam_rows, max_views, table, n_rows, table_kind,
                            n_points, n, max_iters, points, points_f32, point_stride, info, residual, sqrt_info, stream);
}

static_assert(UT_LOSS_SQUARED == ut::FITV_LOSS_SQUARED && UT_LOSS_HUBER == ut::FITV_LOSS_HUBER &&
              UT_LOSS_GEMAN_MCCLURE == ut::FITV_LOSS_GEMAN_MCCLURE, "umetrack_hip_robust.h and ut_kernels.h");

namespace {
// The argument checks the four entries in the views share, on the arguments as the kernels get them, in the order the messages
// have always had.  An entry's own checks come second and third in that order, so the entry states them and they are reported
// from here: null_own - a required pointer of its own is NULL; own - the message of its own first broken rule, or null.
int fit_views_args(ut_handle h, const char* who, const ut::FitViewsRobustArgs& a, int table_kind, int flags = FIT_NO_TARGETS,
                   bool null_own = false, const char* own = nullptr) {
  const ut::FitViewsArgs& g = a.views;
  if (!g.window || !g.cam_rows || !g.table || null_own) return fail_as(h, who, "null argument");
  if (own) return fail_as(h, who, own);
  if (table_kind != UT_CAMERA_FISHEYE62 && table_kind != UT_CAMERA_PINHOLE)
    return fail_as(h, who, "table_kind must be UT_CAMERA_FISHEYE62 or UT_CAMERA_PINHOLE");
  if (g.max_views < 1 || g.max_views > UT_TRI_MAX_VIEWS) return fail_as(h, who, "max_views must be in 1..UT_TRI_MAX_VIEWS (8)");
  if (g.n_rows < 1) return fail_as(h, who, "bad argument");
  if (a.loss != UT_LOSS_SQUARED && a.loss != UT_LOSS_HUBER && a.loss != UT_LOSS_GEMAN_MCCLURE)
    return fail_as(h, who, "loss must be UT_LOSS_SQUARED, UT_LOSS_HUBER or UT_LOSS_GEMAN_MCCLURE");
  if (a.loss != UT_LOSS_SQUARED && (!(a.loss_scale > 0.f) || !(a.loss_scale <= 3.0e38f)))
    return fail_as(h, who, "loss_scale must be positive and finite");
  return fit_pose_args(h, who, g.pose, flags);
}

// What follows the checks of an entry in the views: nothing for n = 0; the windows' device against the handle's; the status words,
// the device, the status word into the arguments; `launch` (it returns the entry's code); the index check's answer if synchronous.
extern "C++" template <class Launch>
int launch_in_views(ut_handle h, const char* who, ut::FitViewsArgs& g, void* stream, Launch launch) {
  if (g.pose.n == 0) return UT_OK;
  if (h) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, g.window) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device != h->device)
      return fail_as(h, who, "the windows live on another device than the handle");
  }
  StatusTarget st;
  const int rs = status_target(h, &st);
  if (rs) return rs;
  DeviceScope scope(st.device);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  hipStream_t s = (hipStream_t)stream;
  g.status = st.dev;
  const int rc = launch(s);
  if (rc) return rc;
  return st.mode == UT_CHECK_SYNC ? check_status(h, st.dev, st.host, s, who) : UT_OK;
}

int camera_kind(int table_kind) { return table_kind == UT_CAMERA_FISHEYE62 ? ut::PROJECT_FISHEYE62 : ut::PROJECT_PINHOLE; }

// ut_fit_pose_views and ut_fit_pose_views_robust: launch_fit_pose_views_robust hands UT_LOSS_SQUARED without `inlier` on to fit_views.hip
int fit_pose_views_robust(ut_handle h, const char* who, int table_kind, void* stream, ut::FitViewsRobustArgs a) {
  const int rc = fit_views_args(h, who, a, table_kind);
  if (rc) return rc;
  return launch_in_views(h, who, a.views, stream, [&](hipStream_t s) -> int {
    HIPCHK(h, ut::launch_fit_pose_views_robust(a, s)); return UT_OK; });
}
}  // namespace

int ut_fit_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                      const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind, const float* limits,
                      const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                      const int64_t* mirror, float t_scale, int max_iters, int n, float* joint_angles, int ja_stride,
                      float* wrist_xf, int xf_stride, float* info, float* residual, void* stream) {
  return fit_pose_views_robust(h, "ut_fit_pose_views", table_kind, stream,
                               {{{hand_model, n_models, nullptr, 0, limits, init_angles, init_ja_stride, init_wrist_xf, init_xf_stride,
                                  mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                                 window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), info, residual, nullptr},
                                UT_LOSS_SQUARED, 0.f, nullptr});
}

int ut_fit_pose_views_robust(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                             const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                             const float* limits, const float* init_angles, int init_ja_stride, const float* init_wrist_xf,
                             int init_xf_stride, const int64_t* mirror, float t_scale, int max_iters, int loss, float loss_scale,
                             int n, float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info,
                             float* residual, float* inlier, void* stream) {
  return fit_pose_views_robust(h, "ut_fit_pose_views_robust", table_kind, stream,
                               {{{hand_model, n_models, nullptr, 0, limits, init_angles, init_ja_stride, init_wrist_xf, init_xf_stride,
                                  mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                                 window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), info, residual, nullptr},
                                loss, loss_scale, inlier});
}

int ut_fit_pose_views_scale(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                            const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                            const float* limits, const float* init_scale, int scale_mode, const float* init_angles,
                            int init_ja_stride, const float* init_wrist_xf, int init_xf_stride, const int64_t* mirror, float t_scale,
                            int max_iters, int loss, float loss_scale, int n, float* joint_angles, int ja_stride, float* wrist_xf,
                            int xf_stride, float* scale, float* info, float* residual, float* inlier, void* stream) {
  const char* who = "ut_fit_pose_views_scale";      // every loss is fit_views_scale.hip's; info is [n,6]
  ut::FitViewsScaleArgs b{{{{hand_model, n_models, nullptr, 0, limits, init_angles, init_ja_stride, init_wrist_xf, init_xf_stride,
                             mirror, t_scale, max_iters, n, joint_angles, ja_stride, wrist_xf, xf_stride},
                            window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), info, residual, nullptr},
                           loss, loss_scale, inlier},
                          init_scale, scale_mode, scale};
  const int rc = fit_views_args(h, who, b.robust, table_kind, FIT_NO_TARGETS, !scale, scale_mode == UT_SCALE_FREE || scale_mode == UT_SCALE_FIXED
                                ? nullptr : "scale_mode must be UT_SCALE_FREE or UT_SCALE_FIXED");
  if (rc) return rc;
  return launch_in_views(h, who, b.robust.views, stream, [&](hipStream_t s) -> int {
    HIPCHK(h, ut::launch_fit_pose_views_scale(b, s)); return UT_OK; });
}

static_assert(UT_COV_OK == ut::COV_OK && UT_COV_SINGULAR == ut::COV_SINGULAR && UT_COV_REFUSED == ut::COV_REFUSED &&
              UT_COV_REFUSED == UT_FIT_REFUSED && UT_COV_MIN_PIVOT == ut::COV_MIN_PIVOT, "umetrack_hip_uncertainty.h and ut_kernels.h");

int ut_pose_information_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                              const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                              const float* angle_sigma, const float* joint_angles, int ja_stride, const float* wrist_xf,
                              int xf_stride, const int64_t* mirror, float t_scale, int loss, float loss_scale, int n,
                              float* pose_info, float* pivot, float* param_sigma, float* landmark_cov, float* info,
                              void* stream) {
  const char* who = "ut_pose_information_views";      // the pose stands where the fits have their start; there are no pose outputs
  ut::PoseInfoViewsArgs b{{{{hand_model, n_models, nullptr, 0, nullptr, joint_angles, ja_stride, wrist_xf, xf_stride, mirror, t_scale,
                             0, n, nullptr, 0, nullptr, 0},
                            window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), nullptr, nullptr, nullptr},
                           loss, loss_scale, nullptr},
                          angle_sigma, pose_info, pivot, param_sigma, landmark_cov, info};
  const int rc = fit_views_args(h, who, b.robust, table_kind, FIT_NO_TARGETS | FIT_POSE_IS_INPUT, false,
                                pose_info || pivot || param_sigma || landmark_cov || info ? nullptr : "all five outputs are NULL");
  if (rc) return rc;
  return launch_in_views(h, who, b.robust.views, stream, [&](hipStream_t s) -> int {
    HIPCHK(h, ut::launch_pose_information_views(b, s)); return UT_OK; });
}

static_assert(UT_SMOOTH_OK == ut::SMOOTH_OK && UT_SMOOTH_GAP == ut::SMOOTH_GAP && UT_SMOOTH_SINGULAR == ut::SMOOTH_SINGULAR &&
              UT_SMOOTH_REFUSED == ut::SMOOTH_REFUSED && UT_SMOOTH_REFUSED == UT_FIT_REFUSED && UT_SMOOTH_WORK == ut::SMOOTH_WORK,
              "umetrack_hip_smooth.h and ut_kernels.h");

int ut_smooth_pose_sequence(ut_handle h, const float* joint_angles, int ja_stride, const float* wrist_xf, int xf_stride,
                            const float* pose_info, const float* pivot, const float* frame_weight, const int32_t* lengths,
                            const float* centre, const float* step_var, int n_var, float t_scale, int n_seq, int n_frames,
                            float* workspace, float* joint_angles_out, int ja_out_stride, float* wrist_xf_out, int xf_out_stride,
                            float* param_sigma, float* info, void* stream) {
  // stateless like ut_fit_pose: h may be NULL
  const char* who = "ut_smooth_pose_sequence";
  if (!joint_angles || !wrist_xf) return fail_as(h, who, "joint_angles and wrist_xf are required");
  if (!pose_info || !pivot) return fail_as(h, who, "pose_info and pivot are required");
  if (!step_var) return fail_as(h, who, "step_var is required");
  if (!workspace) return fail_as(h, who, "workspace is required");
  if (!joint_angles_out || !wrist_xf_out) return fail_as(h, who, "joint_angles_out and wrist_xf_out are required");
  if (ja_stride < 22 || xf_stride < 12 || ja_out_stride < 22 || xf_out_stride < 12)
    return fail_as(h, who, "a stride is below 22 (angles) / 12 (wrist)");
  if (n_seq < 0) return fail_as(h, who, "n_seq is negative");
  if (n_frames < 1) return fail_as(h, who, "n_frames must be at least 1");
  if (n_var != 1 && n_var != n_seq) return fail_as(h, who, "n_var must be 1 or n_seq");
  if (!(t_scale > 0.f) || !(t_scale <= 3.0e38f)) return fail_as(h, who, "t_scale must be positive and finite");
  if (n_seq == 0) return UT_OK;
  const ut::SmoothArgs a{joint_angles, ja_stride, wrist_xf, xf_stride, pose_info, pivot, frame_weight, lengths, centre, step_var, n_var,
                         t_scale, n_seq, n_frames, workspace, joint_angles_out, ja_out_stride, wrist_xf_out, xf_out_stride,
                         param_sigma, info};
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_smooth_pose_sequence(a, (hipStream_t)stream));
  return UT_OK;
}

static_assert(UT_START_MAX_SEEDS == 64, "one lane per seed");

int ut_start_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                        const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                        const float* limits, const float* bank_angles, int n_bank, const double* seeds, int n_seeds,
                        const int64_t* mirror, float t_scale, int iters, int n,
                        float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride, float* info, void* stream) {
  const char* who = "ut_start_pose_views";      // there is no start to require and no max_iters: the checks of the fits, restated
  if (!hand_model || !window || !cam_rows || !table || !bank_angles || !seeds || !joint_angles || !wrist_xf)
    return fail_as(h, who, "null argument");
  if (table_kind != UT_CAMERA_FISHEYE62 && table_kind != UT_CAMERA_PINHOLE)
    return fail_as(h, who, "table_kind must be UT_CAMERA_FISHEYE62 or UT_CAMERA_PINHOLE");
  if (max_views < 1 || max_views > UT_TRI_MAX_VIEWS) return fail_as(h, who, "max_views must be in 1..UT_TRI_MAX_VIEWS (8)");
  if (n < 0 || n_rows < 1 || (n_models != 1 && n_models != n)) return fail_as(h, who, "bad argument");
  if (n_bank < 1 || (long long)n * n_bank > 0x7fffffffLL) return fail_as(h, who, "n_bank must be at least 1 and n * n_bank fit an int");
  if (n_seeds < 1 || n_seeds > UT_START_MAX_SEEDS) return fail_as(h, who, "n_seeds must be in 1..UT_START_MAX_SEEDS (64)");
  if (iters < 1 || iters > 256) return fail_as(h, who, "iters must be in 1..256");
  if (ja_stride < 22 || xf_stride < 12) return fail_as(h, who, "a stride is below 22 (angles) / 12 (wrist)");
  if (!(t_scale > 0.f) || !(t_scale <= 3.0e38f)) return fail_as(h, who, "t_scale must be positive and finite");
  ut::StartViewsArgs a{{{hand_model, n_models, nullptr, 0, limits, nullptr, 0, nullptr, 0, mirror, t_scale, 0, n, joint_angles, ja_stride,
                         wrist_xf, xf_stride},
                        window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), info, nullptr, nullptr},
                       bank_angles, n_bank, seeds, n_seeds, iters};
  return launch_in_views(h, who, a.views, stream, [&](hipStream_t s) -> int {
    HIPCHK(h, ut::launch_start_pose_views(a, s)); return UT_OK; });
}

int ut_select_pose(const float* joint_angles, int ja_stride, const float* wrist_xf, int xf_stride, const float* info,
                   int n, int n_cand, float* out_angles, int out_ja_stride, float* out_wrist_xf, int out_xf_stride,
                   float* out_info, int32_t* out_index, void* stream) {
  const char* who = "ut_select_pose";      // no handle: the device is the caller's current one, as for ut_fit_pose with h == NULL
  if (!joint_angles || !wrist_xf || !info || !out_angles || !out_wrist_xf) return fail_as(nullptr, who, "null argument");
  if (n < 0 || n_cand < 1 || (long long)n * n_cand > 0x7fffffffLL) return fail_as(nullptr, who, "bad argument");
  if (ja_stride < 22 || xf_stride < 12 || out_ja_stride < 22 || out_xf_stride < 12)
    return fail_as(nullptr, who, "a stride is below 22 (angles) / 12 (wrist)");
  if (n == 0) return UT_OK;
  const ut::SelectPoseArgs a{joint_angles, ja_stride, wrist_xf, xf_stride, info, n, n_cand, out_angles, out_ja_stride, out_wrist_xf,
                             out_xf_stride, out_info, out_index};
  HIPCHK(nullptr, ut::launch_select_pose(a, (hipStream_t)stream));
  return UT_OK;
}

static_assert(UT_TRACK_WARM == ut::TRACK_WARM && UT_TRACK_COLD == ut::TRACK_COLD && UT_TRACK_NONE == ut::TRACK_NONE,
              "umetrack_hip_track.h and ut_kernels.h");

int ut_track_pose_views(ut_handle h, const float* hand_model, int n_models, const double* window, const float* weights,
                        const int32_t* cam_rows, int max_views, const double* table, int n_rows, int table_kind,
                        const float* limits,
                        const float* init_angles, int init_ja_stride, const float* init_wrist_xf, int init_xf_stride,
                        const float* cold_angles, int cold_ja_stride, const float* cold_wrist_xf, int cold_xf_stride,
                        const float* cold_info, const int32_t* cold_index, double recover_ratio, double recover_floor,
                        const int32_t* lengths, const int64_t* mirror, float t_scale, int max_iters, int loss, float loss_scale,
                        int n_seq, int n_frames, float* joint_angles, int ja_stride, float* wrist_xf, int xf_stride,
                        float* info, int32_t* chosen, void* stream) {
  const char* who = "ut_track_pose_views";      // the checks of the fits on n = n_seq * n_frames rows; its own come second and third
  const bool rows_ok = n_seq >= 0 && n_frames >= 1 && (long long)n_seq * n_frames <= 0x7fffffffLL;
  const int n_cold = (cold_angles != nullptr) + (cold_wrist_xf != nullptr) + (cold_info != nullptr) + (cold_index != nullptr);
  const char* own = nullptr;
  if (!rows_ok) own = "n_seq must not be negative, n_frames at least 1, and n_seq * n_frames fit an int";
  else if ((init_angles == nullptr) != (init_wrist_xf == nullptr)) own = "init_angles and init_wrist_xf must both be given or both be NULL";
  else if (n_cold != 0 && n_cold != 4) own = "cold_angles, cold_wrist_xf, cold_info and cold_index must all be given or all be NULL";
  else if (!init_angles && !n_cold) own = "neither an init nor cold arrays: there is nothing to start from";
  else if (n_cold && (cold_ja_stride < 22 || cold_xf_stride < 12)) own = "a stride is below 22 (angles) / 12 (wrist)";
  else if (!(recover_ratio >= 1.0) || !(recover_ratio <= 1.7e308)) own = "recover_ratio must be finite and at least 1";
  else if (!(recover_floor >= 0.0) || !(recover_floor <= 1.7e308)) own = "recover_floor must be finite and not negative";
  ut::TrackViewsArgs a{{{{hand_model, n_models, nullptr, 0, limits, init_angles, init_ja_stride, init_wrist_xf, init_xf_stride, mirror, t_scale,
                          max_iters, rows_ok ? n_seq * n_frames : 0, joint_angles, ja_stride, wrist_xf, xf_stride},
                         window, weights, cam_rows, max_views, table, n_rows, camera_kind(table_kind), info, nullptr, nullptr},
                        loss, loss_scale, nullptr},
                       cold_angles, cold_ja_stride, cold_wrist_xf, cold_xf_stride, cold_info, cold_index, recover_ratio, recover_floor,
                       lengths, n_seq, n_frames, chosen};
  const int rc = fit_views_args(h, who, a.robust, table_kind, FIT_NO_TARGETS | FIT_START_OPTIONAL, !info || !chosen, own);
  if (rc) return rc;
  return launch_in_views(h, who, a.robust.views, stream, [&](hipStream_t s) -> int {
    HIPCHK(h, ut::launch_track_pose_views(a, s)); return UT_OK; });
}

static_assert(UT_RENDER_MAX_VERTICES == ut::RENDER_MAX_VERTICES && UT_RENDER_MAX_VERTICES <= UT_MESH_MAX_VERTICES, "vertex cap");

int ut_render_mesh(ut_handle h, const ut_mesh* mesh, const float* vertices, const double* crop_params, int n_crops,
                   const int64_t* sample_range, int n, int crop_size, float* depth, int32_t* tri, uint8_t* shade,
                   void* stream) {
  if (!mesh) return fail(h, UT_E_INVALID, "ut_render_mesh: null mesh");
  if (h && h->device != mesh->device) return fail(h, UT_E_INVALID, "ut_render_mesh: the mesh lives on another device than the handle");
  if (mesh->n_triangles <= 0) return fail(h, UT_E_INVALID, "ut_render_mesh: the mesh has no triangles");
  if (crop_size != ut::RENDER_CROP) return fail(h, UT_E_UNSUPPORTED, "ut_render_mesh: crop_size must be 96");
  if (mesh->n_vertices > UT_RENDER_MAX_VERTICES) {
    char msg[200];
    snprintf(msg, sizeof msg, "ut_render_mesh: %d vertices, more than UT_RENDER_MAX_VERTICES (%d) that fit a workgroup's LDS next "
             "to the depth plane", mesh->n_vertices, UT_RENDER_MAX_VERTICES);
    return fail(h, UT_E_UNSUPPORTED, msg);
  }
  if (n < 0 || n_crops < 0) return fail(h, UT_E_INVALID, "ut_render_mesh: bad argument");
  if (n == 0) return UT_OK;
  if (!vertices || !crop_params || !sample_range) return fail(h, UT_E_INVALID, "ut_render_mesh: null argument");
  if (((uintptr_t)depth | (uintptr_t)tri | (uintptr_t)shade) & 15)
    return fail(h, UT_E_INVALID, "ut_render_mesh: depth, tri and shade must be 16-byte aligned");
  DeviceScope scope(mesh->device);
  if (scope.err != hipSuccess) return fail(h, UT_E_HIP, "hipSetDevice", scope.err);
  StatusTarget st;
  int rc = status_target(h, &st);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  ut::RenderArgs g{};
  g.vertices = vertices; g.nv = mesh->n_vertices; g.tris = (const int4*)mesh->tris; g.nt = mesh->n_triangles;
  g.crop_params = crop_params; g.sample_range = sample_range; g.n = n; g.n_crops = n_crops;
  g.depth = depth; g.tri = tri; g.shade = shade; g.status = st.dev;
  HIPCHK(h, ut::launch_render_check(g, s));
  if (st.mode == UT_CHECK_SYNC && (rc = check_status(h, st.dev, st.host, s, "ut_render_mesh"))) return rc;
  HIPCHK(h, ut::launch_render_mesh(g, s));
  return UT_OK;
}

int ut_gen_crop_cameras(ut_handle h, const double* cam_params, const double* camera_angles, const float* hand_model,
                        const float* joint_limits, int n_models, const float* joint_angles, const float* wrist_xf,
                        const int32_t* frame_idx, const int64_t* hand_idx, int n, int n_cams, int max_views, int min_vis,
                        int src_w, int src_h, int crop_size, double focal_multiplier, double* crop_params,
                        float* intrinsics, float* extrinsics, int32_t* cam_index, int32_t* n_views, int32_t* status,
                        float* landmarks, void* stream) {
  if (n == 0) return UT_OK;
  if (!cam_params || !camera_angles || !hand_model || !joint_limits || !joint_angles || !wrist_xf || !frame_idx ||
      !hand_idx || !crop_params || !intrinsics || !extrinsics || !cam_index || !n_views || !status || n < 0 ||
      (n_models != 1 && n_models != n) || n_cams <= 0 || max_views <= 0 || src_w <= 0 || src_h <= 0 || crop_size <= 1)
    return fail(h, UT_E_INVALID, "ut_gen_crop_cameras: bad argument");
  ON_DEVICE_IF(h);
  ut::CropGenArgs g{};
  g.cam_params = cam_params; g.camera_angles = camera_angles; g.hand_model = hand_model; g.joint_limits = joint_limits;
  g.joint_angles = joint_angles; g.wrist_xf = wrist_xf; g.frame_idx = frame_idx; g.hand_idx = hand_idx;
  g.n = n; g.n_models = n_models; g.n_cams = n_cams; g.max_views = max_views; g.min_vis = min_vis;
  g.src_w = src_w; g.src_h = src_h; g.crop_size = crop_size; g.focal_multiplier = focal_multiplier;
  g.crop_params = crop_params; g.intrinsics = intrinsics; g.extrinsics = extrinsics; g.cam_index = cam_index;
  g.n_views = n_views; g.status = status; g.landmarks = landmarks;
  HIPCHK(h, ut::launch_cropgen(g, (hipStream_t)stream));
  return UT_OK;
}

int ut_gen_crop_cameras_from_window_points(ut_handle h, const double* cam_params, int n_cam_rows, const double* keypoints,
                                           const int32_t* src_row, const int64_t* hand_idx, int n, int max_views,
                                           int crop_size, double focal_multiplier, double* crop_params, float* intrinsics,
                                           float* extrinsics, int32_t* cam_index, int32_t* n_views, int32_t* status,
                                           void* stream) {
  if (n == 0) return UT_OK;
  if (!cam_params || !keypoints || !src_row || !hand_idx || !crop_params || !intrinsics || !extrinsics || !cam_index ||
      !n_views || !status || n < 0 || n_cam_rows <= 0 || max_views < 1 || max_views > 3 || crop_size <= 1)
    return fail(h, UT_E_INVALID, "ut_gen_crop_cameras_from_window_points: bad argument");
  ON_DEVICE_IF(h);
  // the index arrays are read back and checked before anything is launched: a bad row is reported, never read
  std::vector<int32_t> rows((size_t)n * max_views);
  std::vector<int64_t> hands((size_t)n);
  HIPCHK(h, hipMemcpyAsync(rows.data(), src_row, rows.size() * sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream));
  HIPCHK(h, hipMemcpyAsync(hands.data(), hand_idx, hands.size() * sizeof(int64_t), hipMemcpyDefault, (hipStream_t)stream));
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  for (int32_t r : rows)
    if (r < -1 || r >= n_cam_rows)
      return fail(h, UT_E_INVALID, "ut_gen_crop_cameras_from_window_points: src_row outside [-1, n_cam_rows)");
  for (int64_t x : hands)
    if (x != 0 && x != 1) return fail(h, UT_E_INVALID, "ut_gen_crop_cameras_from_window_points: hand_idx not 0 or 1");
  ut::CropGenWindowArgs g{};
  g.cam_params = cam_params; g.keypoints = keypoints; g.src_row = src_row; g.hand_idx = hand_idx;
  g.n = n; g.max_views = max_views; g.crop_size = crop_size; g.focal_multiplier = focal_multiplier;
  g.crop_params = crop_params; g.intrinsics = intrinsics; g.extrinsics = extrinsics; g.cam_index = cam_index;
  g.n_views = n_views; g.status = status;
  HIPCHK(h, ut::launch_cropgen_window(g, (hipStream_t)stream));
  return UT_OK;
}

int ut_gen_crop_matrices(ut_handle h, const float* orig_extrinsics, const float* orig_intrinsics, const float* crop_points,
                         const int64_t* hand_idx, int n_frames, int n_views, int n_pts, int crop_size,
                         double focal_multiplier, float* extrinsics_xf, float* new_intrinsics, float* resample_xf,
                         int32_t* status, void* stream) {
  if (n_frames == 0 || n_views == 0) return UT_OK;
  if (!orig_extrinsics || !orig_intrinsics || !crop_points || !hand_idx || !extrinsics_xf || !new_intrinsics ||
      !resample_xf || !status || n_frames < 0 || n_views < 0 || n_pts <= 0 || crop_size <= 1)
    return fail(h, UT_E_INVALID, "ut_gen_crop_matrices: bad argument");
  ON_DEVICE_IF(h);
  ut::CropMatArgs g{};
  g.orig_extrinsics = orig_extrinsics; g.orig_intrinsics = orig_intrinsics; g.crop_points = crop_points;
  g.hand_idx = hand_idx; g.n_frames = n_frames; g.n_views = n_views; g.n_pts = n_pts; g.crop_size = crop_size;
  g.focal_multiplier = focal_multiplier; g.extrinsics_xf = extrinsics_xf; g.new_intrinsics = new_intrinsics;
  g.resample_xf = resample_xf; g.status = status;
  HIPCHK(h, ut::launch_cropmat(g, (hipStream_t)stream));
  return UT_OK;
}

int ut_resample_homography(ut_handle h, const void* src, int src_is_f32, int n, int src_h, int src_w,
                           const float* resample_xf, int out_h, int out_w, float* out, void* stream) {
  if (n == 0) return UT_OK;
  if (!src || !resample_xf || !out || n < 0 || src_h < 2 || src_w < 2 || out_h <= 0 || out_w <= 0)
    return fail(h, UT_E_INVALID, "ut_resample_homography: bad argument");
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_resample_homography(src, src_is_f32, n, src_h, src_w, resample_xf, out_h, out_w, out,
                                           (hipStream_t)stream));
  return UT_OK;
}

int ut_keypoint_metrics(ut_handle h, const float* gt, const float* tracked, const uint8_t* valid, int n_hands, int n_frames,
                        double* err, double* acc, double* gt_acc, uint8_t* valid_acc, void* stream) {
  if (n_hands == 0 || n_frames == 0) return UT_OK;
  if (!gt || !tracked || !valid || !err || n_hands < 0 || n_frames < 0 ||
      (n_frames >= 3 && (!acc || !gt_acc || !valid_acc)))
    return fail(h, UT_E_INVALID, "ut_keypoint_metrics: bad argument");
  ON_DEVICE_IF(h);
  HIPCHK(h, ut::launch_keypoint_metrics(gt, tracked, valid, n_hands, n_frames, err, acc, gt_acc, valid_acc,
                                        (hipStream_t)stream));
  return UT_OK;
}

int ut_set_backbone_lanes(ut_handle h, int lanes) {
  if (!h || (lanes != 1 && lanes != 2)) return fail(h, UT_E_INVALID, "ut_set_backbone_lanes: 1 or 2");
  h->lanes = lanes;
  return UT_OK;
}

int ut_set_conv_arithmetic(ut_handle h, int mode) {
  if (!h || (mode != UT_CONV_FP32 && mode != UT_CONV_SPLIT_F16 && mode != UT_CONV_SPLIT_F16_ALWAYS)) return fail(h, UT_E_INVALID, "ut_set_conv_arithmetic: bad argument");
  h->conv_arith = mode;
  if (mode != UT_CONV_FP32 && h->scale_mode != UT_SPLIT_SCALE_DYNAMIC && !h->calibrated) {
    ON_DEVICE_OF(h);
    return calibrate_builtin(h);
  }
  return UT_OK;
}

int ut_set_block_fusion(ut_handle h, int on) {
  if (!h) return UT_E_INVALID;
  h->block_fusion = on != 0;
  return UT_OK;
}

int ut_set_resident_weights(ut_handle h, int on) {
  if (!h) return UT_E_INVALID;
  if (on < 0 || on > 7) return fail(h, UT_E_INVALID, "ut_set_resident_weights: bad argument");
  h->resident_weights = on;
  return UT_OK;
}

int ut_set_latency_mode(ut_handle h, int on) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  if (on && !h->splitk_ws) {
    const size_t n = 1u << 20;          // 4 MB: S x M x cout of every few-crop layer of this network is 442 k floats
    int rc;
    if ((rc = dev_alloc(h, &h->splitk_ws, n)) || (rc = dev_alloc(h, &h->zero_bias, 256))) return rc;
    HIPCHK(h, hipMemset(h->zero_bias, 0, 256 * sizeof(float)));
    h->splitk_floats = n;
  }
  h->latency_mode = on != 0;
  return UT_OK;
}

int ut_set_index_checks(ut_handle h, int mode) {
  if (!h || (mode != UT_CHECK_SYNC && mode != UT_CHECK_DEFERRED)) return fail(h, UT_E_INVALID, "ut_set_index_checks: bad argument");
  h->check_mode = mode;
  return UT_OK;
}

int ut_poll_status(ut_handle h, void* stream) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  return check_status(h, h->status, h->status_host, (hipStream_t)stream, "reported late (deferred checks)");
}

int ut_status_snapshot(ut_handle h, int32_t* dst, void* stream) {
  if (!h || !dst) return fail(h, UT_E_INVALID, "ut_status_snapshot: null argument");
  ON_DEVICE_OF(h);
  HIPCHK(h, hipMemcpyAsync(dst, h->status, 2 * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return UT_OK;
}

int ut_profile_begin(ut_handle h, void* stream) {
  if (!h) return UT_E_INVALID;
  (void)stream;
  ON_DEVICE_OF(h);
  prof_clear(h);
  h->profiling = true;
  return UT_OK;
}

int ut_profile_end(ut_handle h, void* stream, double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total) {
  if (!h) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  double ms[2], fl[2];
  int64_t n[2];
  int rc = prof_reduce(h, (hipStream_t)stream, ms, n, fl);
  if (rc) return rc;
  if (conv_ms_total) *conv_ms_total = ms[0] + ms[1];
  if (conv_launches) *conv_launches = n[0] + n[1];
  if (conv_flops_total) *conv_flops_total = fl[0] + fl[1];
  return UT_OK;
}

int ut_profile_end_by_kind(ut_handle h, void* stream, double* ms2, int64_t* launches2, double* flops2) {
  if (!h || !ms2 || !launches2 || !flops2) return UT_E_INVALID;
  ON_DEVICE_OF(h);
  return prof_reduce(h, (hipStream_t)stream, ms2, launches2, flops2);
}

}  // extern "C"
