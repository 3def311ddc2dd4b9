// mivod CDNA4 (gfx950) kernel helpers: dtype tags, 8-wide vector load/store
// with fused conversion, the scale-then-cast helpers of the flat kernels, wave64 reductions, the dropout hash, the CU count.  What only
// the matrix-core kernels share (MFMA, LDS swizzles, transposed reads, LDS-DMA) is in
// mv_mfma.h, which includes this header.
//
// Every memory-bound mivod kernel moves 8 elements per lane per step: 16 B for
// bf16/fp16 (one global_load_dwordx4) and 32 B for fp32 (two dwordx4).  The
// conversion to/from bf16 uses gfx950's v_cvt_pk_bf16_f32 (RNE), emitted by
// clang for a plain (__bf16) cast on this target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mv {

enum Dtype : int { F32 = 0, BF16 = 1, F16 = 2 };

constexpr int kWave = 64;
constexpr int kVec = 8;            // elements per lane per step
constexpr int kBlock = 256;        // 4 waves
constexpr int kChunk = 4096;       // elements per workgroup (2 steps of 256x8)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// Compute units of the current device (256 if the query fails), asked once per process:
// the persistent kernels size their grids by it.
inline int num_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
      v = 256;
    return v;
  }();
  return n;
}

template <typename T> struct DT;
template <> struct DT<float> { static constexpr Dtype v = F32; };
template <> struct DT<__bf16> { static constexpr Dtype v = BF16; };
template <> struct DT<_Float16> { static constexpr Dtype v = F16; };

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(__bf16 x) { return (float)x; }
__device__ __forceinline__ float to_f32(_Float16 x) { return (float)x; }

template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ __bf16 from_f32<__bf16>(float x) { return (__bf16)x; }
template <> __device__ __forceinline__ _Float16 from_f32<_Float16>(float x) { return (_Float16)x; }

// ---- 8-wide vector load (aligned) -> fp32 registers ----
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  f32x4 a = *reinterpret_cast<const f32x4*>(p);
  f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
  v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
__device__ __forceinline__ void load8(const __bf16* p, float (&v)[8]) {
  u16x8 a = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(((uint32_t)a[j]) << 16);
}
// non-temporal (last-use) streaming load: the line is not kept in L2 / MALL
__device__ __forceinline__ void load8_nt(const __bf16* p, float (&v)[8]) {
  u16x8 a = __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(p));
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(((uint32_t)a[j]) << 16);
}
__device__ __forceinline__ void load8(const _Float16* p, float (&v)[8]) {
  u16x8 a = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned short s = a[j];
    v[j] = (float)__builtin_bit_cast(_Float16, s);
  }
}

// ---- fp32 registers -> 8-wide vector store (aligned), with conversion ----
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  f32x4 a = {v[0], v[1], v[2], v[3]};
  f32x4 b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}
// Packed RNE f32x2 -> bf16x2 on gfx950 (lo <- a, hi <- b).  Two forms:
//
// cvt_pk_bf16: inline asm.  NOT __builtin_convertvector(f32x2 -> bf16x2): ROCm 7.2
//   clang mis-lowers that inside unrolled loops (only the even elements converted:
//   caught by tests/test_kernels_gpu.py::test_pack_unpack_cast_scale).  The compiler's
//   hazard recognizer cannot see into inline asm, so its inputs must NOT be fresh MFMA
//   results in VGPRs: CDNA needs 11 wait states (16x16x32) between an MFMA writing a
//   VGPR and a VALU reading it and does not interlock.  Every use in mivod reads values
//   that went through VALU epilogue math or an accvgpr read first —
//   scripts/check_mfma_asm_hazards.py (tests/test_kernel_asm_hazards.py) verifies that
//   for every kernel.  (Round 2's stem_fwd_kernel NaN at __launch_bounds__(256, 2) was
//   this hazard: its accumulators moved to VGPRs and were converted 0-6 wait states
//   after the MFMA.)
// cvt_pk_bf16_cc: compiler-selected (a two-element build of scalar casts), hazard-safe
//   on raw MFMA accumulators — used there.  Not used everywhere: in the conv3x3 / GEMM
//   epilogues it changed the register allocation and cost the 128x128 conv3x3 tiles
//   ~45% (7.6 -> 11.1 ms/step at bs 2048, round-3 A/B, gpurun_out/ab_new.md).
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t cvt_pk_bf16_cc(float a, float b) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ void store8(__bf16* p, const float (&v)[8]) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 o = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]),
             cvt_pk_bf16(v[6], v[7])};
  *reinterpret_cast<u32x4*>(p) = o;
}
__device__ __forceinline__ void store8(_Float16* p, const float (&v)[8]) {
  u16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = __builtin_bit_cast(unsigned short, (_Float16)v[j]);
  *reinterpret_cast<u16x8*>(p) = o;
}

// scalar tail helpers
template <typename T>
__device__ __forceinline__ float ld1(const T* p) { return to_f32(*p); }
template <typename T>
__device__ __forceinline__ void st1(T* p, float v) { *p = from_f32<T>(v); }

__device__ __forceinline__ bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// the value as the destination dtype stores it (the non-finite check of a pack must see
// an fp16 overflow of the cast, as the overflow guard's scan of the packed bucket would)
template <typename TD>
__device__ __forceinline__ float stored(float x) {
  if constexpr (std::is_same<TD, float>::value) return x;
  else return (float)(TD)x;
}

// x * scale rounded to fp32 before the cast to the destination dtype, as
// (t.float() * scale).to(dst) rounds: left to the compiler, the vector body folds the
// multiply into the f16 conversion (one rounding of the exact product), which differs from
// the scalar paths and from PyTorch wherever the fp32 product is a tie of the destination
// (tests/test_flat_kernels_gpu.py found 8 such elements in 4096).  The empty asm makes the
// fp32 product a value the conversion cannot look through; it emits no instruction.
__device__ __forceinline__ float scaled(float x, float scale) {
  float p = x * scale;
  asm("" : "+v"(p));
  return p;
}

constexpr float kSqrt1_2 = 0.70710678118654752f;
constexpr float kInvSqrt2Pi = 0.39894228040143268f;

// Exact-erf GELU (BERT's), with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7,
// far below bf16's 4e-3 resolution): one reciprocal, a 5-term polynomial and ONE
// exponential, exp(-v^2 / 2), which gelu'(v) reuses for the Gaussian pdf term.  ocml's
// erff is a branchy piecewise rational approximation; with it the bias-GELU passes were
// VALU-bound at ~2.4 TB/s (profiles/r2_bert_large_bs512_short_attn_bwd.md).
__device__ __forceinline__ void gelu_parts(float v, float* cdf, float* e) {
  const float z = fabsf(v) * kSqrt1_2;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, z, 1.f));
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  p *= t;
  *e = __expf(-z * z);                               // exp(-v^2 / 2)
  const float erf_abs = __builtin_fmaf(-p, *e, 1.f);
  *cdf = 0.5f + 0.5f * __builtin_copysignf(erf_abs, v);
}
__device__ __forceinline__ float gelu(float v) {
  float cdf, e;
  gelu_parts(v, &cdf, &e);
  return v * cdf;
}
__device__ __forceinline__ float gelu_grad(float v) {
  float cdf, e;
  gelu_parts(v, &cdf, &e);
  return __builtin_fmaf(v * kInvSqrt2Pi, e, cdf);
}

// lowbias32 integer hash (a bijection of 32 bits): the dropout generators of mv_attn.hip
// and mv_bert.hip, mirrored in Python by tests/test_dropout_stats.py
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// wave64 sum via DPP-backed shuffles
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// Block (256 threads = 4 waves) sum of NV values; result valid in thread 0.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV]) {
  __shared__ float red[NV][kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1);
  const int w = threadIdx.x / kWave;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = wave_sum(v[i]);
    if (lane == 0) red[i][w] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < kBlock / kWave; ++j) s += red[i][j];  // fixed order: deterministic
      v[i] = s;
    }
  }
}

}  // namespace mv
