// What the hand-written convolution kernels (conv_*.hip) share: vector types, buffer-resource words, the LDS-DMA piece, the
// two-piece fp16 split, the tile-queue hand-over word, the accumulator-register constraints of the register-resident kernels
// and the launchers' host tail.  Included after ut_kernels.h.  Everything sits in an anonymous namespace:
// a translation unit has its own copy, so two builds of one kernel (tools/diag patches copies of the sources) link into one
// library.  The device functions are forced inline: sharing them here costs a kernel no instruction.
#pragma once
#include <atomic>
#include <initializer_list>

#include "ut_kernels.h"

namespace ut {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) float lds_f32;

// The four words of a raw buffer descriptor over [base, base + bytes), wave-uniform (stride 0): what the asm LDS-DMA below
// takes as its "s" operand.  A per-lane offset at or beyond `bytes` reads zeros.
__device__ __forceinline__ u32x4 rsrc_words(const void* base, unsigned bytes) {
  const unsigned long long a = (unsigned long long)base;
  u32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
  r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xFFFFu);   // stride 0
  r.z = __builtin_amdgcn_readfirstlane(bytes);
  r.w = 0x00020000u;
  return r;
}

// One LDS-DMA piece: 64 lanes x 16 bytes from a buffer (per-lane byte offset, out-of-range -> zeros) straight into LDS at
// lds_addr + lane * 16.  Inline asm on purpose: with the builtin hipcc treats the pending LDS write as aliasing every ds_read
// and drains vmcnt(0) in front of the fragment reads of the CURRENT buffer, which serialises the whole prefetch.  M0 (the LDS
// base of the transfer) is written in the statement that uses it and restored; the transfer is invisible to the compiler's wait
// counting, so the caller waits on vmcnt itself before the barrier (or counter) that publishes the buffer.
__device__ __forceinline__ void dma_piece(u32x4 rsrc, unsigned lds_addr, unsigned voffset) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voffset), "s"(lds_addr), "s"(rsrc)
      : "memory");
}
// ... + a wave-uniform byte offset in a scalar register (not covered by the descriptor's range check).  An overload, not a
// defaulted argument: the form above encodes a literal 0 where this one names a register.
__device__ __forceinline__ void dma_piece(u32x4 rsrc, unsigned lds_addr, unsigned voffset, unsigned soffset) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voffset), "s"(lds_addr), "s"(rsrc), "s"(soffset)
      : "memory");
}

// The two-piece split every split-fp16 result rests on (conv_split.hip's header has the arithmetic).
// two fp32 values -> their fp16 pieces (first, remainder), each packed {b, a}
__device__ __forceinline__ void split_pair(float a, float b, unsigned& p0, unsigned& p1) {
  const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(a, b));
  const float ra = a - (float)h[0], rb = b - (float)h[1];
  p0 = __builtin_bit_cast(unsigned, h);
  p1 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(ra, rb));
}
// the pieces of a * s and b * s for a power of two s: the products are exact, so fma(a, s, -h) is the remainder (a * s) - h
// in one instruction that also converts h (v_fma_mix_f32)
__device__ __forceinline__ void split_pair_scaled(float a, float b, float s, unsigned& p0, unsigned& p1) {
  const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(a * s, b * s));
  const float ra = __builtin_fmaf(a, s, -(float)h[0]), rb = __builtin_fmaf(b, s, -(float)h[1]);
  p0 = __builtin_bit_cast(unsigned, h);
  p1 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(ra, rb));
}

// Tile-queue hand-over word of a persistent workgroup, at an LDS byte address: one thread writes the next tile's index, every
// wave reads it (wave-uniform) behind a barrier.  Explicit DS instructions: a `volatile int*` into LDS compiles to FLAT
// accesses, which count on vmcnt as well (a read would wait for the tile's stores) and turn every fragment wait of the
// chunk loop into lgkmcnt(0).
__device__ __forceinline__ void slot_write(unsigned lds_addr, int v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(lds_addr), "v"(v) : "memory");
}
__device__ __forceinline__ int slot_read(unsigned lds_addr) {
  int v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr) : "memory");
  return __builtin_amdgcn_readfirstlane(v);
}

// Host: the tail of every launcher here - the dynamic-LDS attribute, the launch, its error.
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (kernel, device): the static word of this template (one per Kernel; SetWith
// names the instantiations that are always set together with it) has one bit per device, and the attribute is set on the first
// launch there.  A device index outside 0..63 has no bit and sets it every time.
template <auto Kernel, auto... SetWith, typename... Args>
hipError_t launch_with_lds(int device, int lds_bytes, int grid, int block, hipStream_t s, const Args&... args) {
  static std::atomic<unsigned long long> attr_set{0};
  const unsigned long long dev_bit = (device >= 0 && device < 64) ? 1ull << device : 0ull;
  if (!dev_bit || !(attr_set.load(std::memory_order_relaxed) & dev_bit)) {
    for (const void* k : {reinterpret_cast<const void*>(Kernel), reinterpret_cast<const void*>(SetWith)...}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
      if (e != hipSuccess) return e;
    }
    attr_set.fetch_or(dev_bit, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds_bytes, s, args...);
  return hipGetLastError();
}

// Host: workgroups of a persistent grid that drains a tile queue - as many as stay resident, never more than tiles
inline int persistent_grid(int num_cu, int n_tiles, int per_cu = 1) {
  return num_cu * per_cu < n_tiles ? num_cu * per_cu : n_tiles;
}

// Host: an fp32 tensor of n x h x w x ch elements that the kernels address with 32-bit byte offsets (buffer descriptors)
inline bool offsets_fit_32(size_t n, size_t h, size_t w, size_t ch) { return n * h * w * ch * sizeof(float) < 0x7FFFFF00ull; }

}  // namespace
}  // namespace ut

// Accumulator-file registers of weight fragment f of a register-resident kernel (conv_c64k.hip, conv_c32s2.hip): a[4 f : 4 f + 3],
// as inline-asm constraints.  Every use pins the fragment to the same physical registers, so the compiler knows they are occupied
// (registers it is not told about it hands to other values) and has no reason to move them (with plain "a" constraints its
// allocator kept shuffling and spilling them).
#define UT_ARF_0 "{a[0:3]}"
#define UT_ARF_1 "{a[4:7]}"
#define UT_ARF_2 "{a[8:11]}"
#define UT_ARF_3 "{a[12:15]}"
#define UT_ARF_4 "{a[16:19]}"
#define UT_ARF_5 "{a[20:23]}"
#define UT_ARF_6 "{a[24:27]}"
#define UT_ARF_7 "{a[28:31]}"
#define UT_ARF_8 "{a[32:35]}"
#define UT_ARF_9 "{a[36:39]}"
#define UT_ARF_10 "{a[40:43]}"
#define UT_ARF_11 "{a[44:47]}"
#define UT_ARF_12 "{a[48:51]}"
#define UT_ARF_13 "{a[52:55]}"
#define UT_ARF_14 "{a[56:59]}"
#define UT_ARF_15 "{a[60:63]}"
#define UT_ARF_16 "{a[64:67]}"
#define UT_ARF_17 "{a[68:71]}"
#define UT_ARF_18 "{a[72:75]}"
#define UT_ARF_19 "{a[76:79]}"
#define UT_ARF_20 "{a[80:83]}"
#define UT_ARF_21 "{a[84:87]}"
#define UT_ARF_22 "{a[88:91]}"
#define UT_ARF_23 "{a[92:95]}"
#define UT_ARF_24 "{a[96:99]}"
#define UT_ARF_25 "{a[100:103]}"
#define UT_ARF_26 "{a[104:107]}"
#define UT_ARF_27 "{a[108:111]}"
#define UT_ARF_28 "{a[112:115]}"
#define UT_ARF_29 "{a[116:119]}"
#define UT_ARF_30 "{a[120:123]}"
#define UT_ARF_31 "{a[124:127]}"
// UT_AR(tap, k-step, plane), all three literal digits: the entry of fragment f = tap * 4 + k-step * 2 + plane - tap picks a row of
// four, (k-step, plane) the entry in it.  Taps 0..7 are register-resident; a kernel whose macros also name tap 8 inside a
// discarded `if constexpr` defines UT_AR_TAP_8 itself.
#define UT_AR_TAP_0 UT_ARF_0, UT_ARF_1, UT_ARF_2, UT_ARF_3
#define UT_AR_TAP_1 UT_ARF_4, UT_ARF_5, UT_ARF_6, UT_ARF_7
#define UT_AR_TAP_2 UT_ARF_8, UT_ARF_9, UT_ARF_10, UT_ARF_11
#define UT_AR_TAP_3 UT_ARF_12, UT_ARF_13, UT_ARF_14, UT_ARF_15
#define UT_AR_TAP_4 UT_ARF_16, UT_ARF_17, UT_ARF_18, UT_ARF_19
#define UT_AR_TAP_5 UT_ARF_20, UT_ARF_21, UT_ARF_22, UT_ARF_23
#define UT_AR_TAP_6 UT_ARF_24, UT_ARF_25, UT_ARF_26, UT_ARF_27
#define UT_AR_TAP_7 UT_ARF_28, UT_ARF_29, UT_ARF_30, UT_ARF_31
#define UT_AR_PICK_00(F0, F1, F2, F3) F0
#define UT_AR_PICK_01(F0, F1, F2, F3) F1
#define UT_AR_PICK_10(F0, F1, F2, F3) F2
#define UT_AR_PICK_11(F0, F1, F2, F3) F3
#define UT_AR_PICK(ROW, S, PL) UT_AR_PICK_##S##PL(ROW)
#define UT_AR(TAP, S, PL) UT_AR_PICK(UT_AR_TAP_##TAP, S, PL)
