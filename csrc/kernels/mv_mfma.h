// The matrix-core kernels' shared device vocabulary: vector types, the MFMA wrapper, the
// XCD workgroup remap, LDS chunk swizzles, gfx950's transposed LDS read, LDS-DMA and the
// counted waits / raw barrier that go with it.  Users: mv_gemm.hip, mv_gemm256.hip,
// mv_conv.hip, mv_conv64.hip, mv_stem.hip, mv_attn.hip.  The address arithmetic of each
// kernel's LDS image stays in its file; what is here is the same in all of them.
#pragma once
#include "mv_common.h"

namespace mv {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));     // one MFMA A / B operand
typedef float f32x4v __attribute__((ext_vector_type(4)));      // one MFMA accumulator
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));       // one transposed LDS read
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- arithmetic, remap
__device__ __forceinline__ f32x4v mfma(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float round_bf16(float x) { return (float)(__bf16)x; }

// bijective XCD-aware remap of the 1-D workgroup id (8 XCDs, round-robin dispatch)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ---------------------------------------------------------------- LDS swizzles
// Row-major tiles of 64-element (128-B) rows read with ds_read_b128: element offset of
// 16-byte chunk ch of row `row`, stored at chunk ch ^ (row & 7) so that the 16 rows of a
// fragment read spread over all banks.
__device__ __forceinline__ int swz64(int row, int ch) { return row * 64 + ((ch ^ (row & 7)) << 3); }

// Chunk XORs of tiles read with the transposed read below (slot (r, ch) holds chunk
// ch ^ f(r)).  A transposed read touches 4 consecutive rows per 16-lane group and rows 8
// apart in the other group of its 32-lane half.
//
// tr_swz4, 128-B rows (mv_conv.hip's weight-gradient stages, mv_stem.hip's dz tile): rows 2
// apart share a bank window on 128-B rows, so {r, r+2, r+8, r+10} get chunk offsets
// {0, 2, 4, 6} (XOR by even values keeps a 32-byte column pair together): conflict-free
// instead of 4-way.
__device__ __forceinline__ int tr_swz4(int r) { return (((r >> 1) & 1) << 1) | (((r >> 3) & 1) << 2); }
// tr_swz8, (row & 3) | (row >> 3 & 1) << 2: the 8 rows {r..r+3, r+8..r+11} one 32-lane
// half reads get 8 distinct values.  mv_attn.hip's Ks image XORs 16-B chunks with it (16
// distinct 16-B bank windows on 128-B rows); mv_gemm256.hip's weight-gradient image (256-B
// rows) XORs in 32-B pairs, tr_swz8 << 1 (8 distinct 32-B windows).
__device__ __forceinline__ int tr_swz8(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }

// ---------------------------------------------------------------- transposed LDS read
// gfx950 ds_read_b64_tr_b16: each 16-lane group reads a 4-row x 16-column block of a
// row-major bf16 LDS array and lane c receives column c of its 4 rows — the k-major MFMA
// operand straight from a row-major image.  Lane c supplies the address of row c / 4,
// columns 4 (c % 4) .. + 3.
__device__ __forceinline__ s16x4 lds_tr4(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
// The same read in inline asm.  hipcc treats the builtin as aliasing every LDS-DMA
// (global_load_lds / buffer_load ... lds) in flight and waits vmcnt(0) before it, so in a
// kernel that prefetches by LDS-DMA the stage issued after the barrier drains before the
// first read: no prefetch at all.  The asm form is invisible to that analysis; its callers
// retire the reads themselves with lds_wait() ahead of their MFMAs.  Kernels without
// LDS-DMA in flight, or with enough workgroups per CU to hide the drain, keep the builtin,
// whose compiler-scheduled reads interleave with the MFMAs.
__device__ __forceinline__ s16x4 lds_tr4_asm(const __bf16* p) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1"
               : "=v"(v)
               : "v"((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p));
  return v;
}
__device__ __forceinline__ void lds_wait() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);     // no MFMA is hoisted above the wait
}

// Two 4-element transposed reads as one MFMA operand, in two forms that are NOT the same
// to the compiler.  cat8_shuffle (a vector shuffle: the register allocator can place the
// halves adjacently): mv_attn.hip, mv_conv64.hip's wgrad64, mv_gemm256.hip's wgrad256.
// cat8_copy (element by element): mv_stem.hip's weight gradient, mv_conv.hip's wgrad3x3 /
// wgrad1x1.  Switching a kernel from one form to the other changes its register
// allocation; which is faster there has not been measured.
__device__ __forceinline__ bf16x8 cat8_shuffle(const s16x4& a, const s16x4& b) {
  const s16x8 o = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, o);
}
__device__ __forceinline__ bf16x8 cat8_copy(const s16x4& a, const s16x4& b) {
  bf16x8 o;
  short* q = reinterpret_cast<short*>(&o);
  q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; q[3] = a[3];
  q[4] = b[0]; q[5] = b[1]; q[6] = b[2]; q[7] = b[3];
  return o;
}

// [rows][64] tile with the tr_swz4 chunk XOR (mv_conv.hip's stages, mv_stem.hip's dz
// tile): lane c of each 16-lane group gets rows r0 .. r0 + 3 of column col0 + c.
template <bool ASM>
__device__ __forceinline__ s16x4 tr4_swz4(const __bf16* base, int r0, int col0, int c) {
  const int r = r0 + (c >> 2), e = col0 + 4 * (c & 3);
  const __bf16* p = base + r * 64 + (((e >> 3) ^ tr_swz4(r)) << 3) + (e & 7);
  if constexpr (ASM) return lds_tr4_asm(p);
  else return lds_tr4(p);
}

// ---------------------------------------------------------------- LDS-DMA
// 16 bytes per lane from global memory into LDS at lds_wave_base + lane * 16, no VGPR round
// trip
__device__ __forceinline__ void glds16(const void* src, __bf16* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0,
                                   0);
}
// The same from a buffer resource at a 32-bit byte offset (an out-of-range offset reads
// zeros).  (A device helper: the builtin written directly in the conv3x3_kernel template
// made the host pass drop its launch stubs.)
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t rs, uint32_t off, __bf16* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(
      rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, off, 0, 0, 0);
}
// Word 3 of a raw buffer descriptor: DATA_FORMAT 32, no swizzle, no index stride — with
// stride 0 the byte offset of every access is range-checked against `bytes`.
constexpr int kRawBufferFlags = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes,
                                           kRawBufferFlags);
}

// ---------------------------------------------------------------- waits and barriers
// Counted wait on outstanding vector-memory operations: LDS-DMA loads issued for later
// stages stay in flight across it.
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_barrier without __syncthreads' vmcnt(0) / lgkmcnt(0) drain, fenced against compiler
// reordering of memory operations
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

}  // namespace mv
