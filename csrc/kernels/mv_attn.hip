// Fused multi-head attention for BERT on gfx950 MFMA: the dense instantiations of the
// kernel templates in mv_attn_kernels.h (the design notes are there), the kernels both
// forms share (delta_kernel, the dropout-mask helper) and the launchers.  Calls with
// segment bounds (AttnParams::seg) go on to mv_attn_seg.hip.
#include "mv_attn_kernels.h"

namespace mv {
namespace attn {

// delta[bh, q] = sum_d dO * O
__global__ __launch_bounds__(256) void delta_kernel(const __bf16* __restrict__ out,
                                                     const __bf16* __restrict__ dout,
                                                     float* __restrict__ delta, int b, int s,
                                                     int h) {
  // 8 lanes per (b, s, h) row, 16 B each: a wave reads 8 whole 128-B rows per load
  // (one-thread-per-row touched 64 lines per instruction and ran at ~1 TB/s)
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const int j8 = (threadIdx.x & 7) * 8;
  const int64_t rows = (int64_t)b * s * h;
  float acc = 0.f;
  if (i < rows) {
    float a[8], e[8];
    load8(out + i * D + j8, a);
    load8(dout + i * D + j8, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a[j] * e[j];
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 4, 64);
  if (i < rows && j8 == 0) {
    const int hi = (int)(i % h);
    const int64_t bs = i / h;
    const int q = (int)(bs % s), bi = (int)(bs / s);
    delta[((int64_t)bi * h + hi) * s + q] = acc;
  }
}

}  // namespace attn
}  // namespace mv

using namespace mv::attn;


void mv_attn_fwd(const AttnParams& p, hipStream_t st) {
  if (p.seg) return mv_attn_seg_fwd(p, st);
  if (p.s <= 2 * KB) {
    // <= 80 VGPRs (6 waves per SIMD, three workgroups per CU): 174 us vs 188 at 82 VGPRs
    // and 181 at 64 (spills) per BERT-Large layer (profiles/r6_ab_log.md)
    hipLaunchKernelGGL((fwd_short_kernel<6, false>), dim3(p.b * p.h), dim3(512), 0, st, p);
    return;
  }
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h);
  hipLaunchKernelGGL(fwd_kernel<false>, grid, dim3(256), 0, st, p);
}

void mv_attn_delta(const AttnParams& p, const void* out, const void* dout, float* delta,
                   hipStream_t st) {
  const int64_t rows = (int64_t)p.b * p.s * p.h;
  static_assert(D == 64, "delta_kernel maps 8 lanes x 8 elements onto a row");
  hipLaunchKernelGGL(delta_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st,
                     (const __bf16*)out, (const __bf16*)dout, delta, p.b, p.s, p.h);
}

void mv_attn_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                 float* dq_part, void* dqkv, hipStream_t st, float* bsum) {
  if (p.s <= 2 * KB) {   // one workgroup per (b, h): no delta / dq_reduce passes
    if (p.seg) return mv_attn_seg_bwd(p, out, dout, delta, dq_part, dqkv, st, bsum);
    hipLaunchKernelGGL(bwd_short_kernel<false>, dim3(p.b * p.h), dim3(512), 0, st, p,
                       (const __bf16*)out, (const __bf16*)dout, (__bf16*)dqkv, bsum);
    return;
  }
  const int64_t rows = (int64_t)p.b * p.s * p.h;
  mv_attn_delta(p, out, dout, delta, st);
  if (p.seg) return mv_attn_seg_bwd(p, out, dout, delta, dq_part, dqkv, st, bsum);
  const int nkb = (p.s + KB - 1) / KB;
  hipLaunchKernelGGL(bwd_kernel<false>, dim3(nkb, p.b * p.h), dim3(256), 0, st, p,
                     (const __bf16*)dout, (const float*)delta, dq_part, (__bf16*)dqkv);
  const int64_t n8 = rows * D / 8;
  hipLaunchKernelGGL(dq_reduce_kernel<false>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0,
                     st, (const float*)dq_part, (__bf16*)dqkv, nkb, p.b, p.s, p.h,
                     p.scale_log2 / LOG2E, (const uint32_t*)nullptr);
}

namespace mv {
namespace attn {
// debug / test helper: materialise the dropout keep-mask [b, h, s(q), s(k)]
__global__ void mask_kernel(int b, int h, int s, uint32_t seed, uint32_t thresh, uint8_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)b * h * s * s;
  if (i >= n) return;
  const int k = (int)(i % s);
  const int q = (int)((i / s) % s);
  const uint32_t bh = (uint32_t)(i / ((int64_t)s * s));
  keep[i] = keep_elem(drop_key(seed, bh), (uint32_t)q, (uint32_t)k, thresh) ? 1 : 0;
}
}  // namespace attn
}  // namespace mv

void mv_attn_dropout_mask(int b, int h, int s, uint32_t seed, uint32_t thresh, uint8_t* keep,
                          hipStream_t st) {
  const int64_t n = (int64_t)b * h * s * s;
  hipLaunchKernelGGL(mv::attn::mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     b, h, s, seed, thresh, keep);
}
