// Causal (lower-triangular) attention: the CAUSAL = true instantiations of the kernel
// templates in mv_attn_kernels.h, dense (<SEG = false>: ranges from lane ids, p.seg never
// read) and within packed runs (<SEG = true>), and their launchers.
// docs/CAUSAL_ATTENTION.md has the contract and the design.
#include "mv_attn_kernels.h"

using namespace mv::attn;

namespace {

template <bool SEG>
void causal_fwd(const AttnParams& p, hipStream_t st) {
  if (p.s <= 2 * KB) {
    hipLaunchKernelGGL((fwd_short_kernel<6, SEG, true>), dim3(p.b * p.h), dim3(512), 0, st, p);
    return;
  }
  // blockIdx.x counts the query blocks down, rotated by (b, h) (fwd_kernel): heavy first
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h);
  hipLaunchKernelGGL((fwd_kernel<SEG, true>), grid, dim3(256), 0, st, p);
}

template <bool SEG>
void causal_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                float* dq_part, void* dqkv, hipStream_t st, float* bsum) {
  if (p.s <= 2 * KB) {   // one workgroup per (b, h): no delta / dq_reduce passes
    hipLaunchKernelGGL((bwd_short_kernel<SEG, true>), dim3(p.b * p.h), dim3(512), 0, st, p,
                       (const __bf16*)out, (const __bf16*)dout, (__bf16*)dqkv, bsum);
    return;
  }
  mv_attn_delta(p, out, dout, delta, st);
  // key block kb runs nkb - kb query blocks: ascending kb is heavy-first as it stands
  const int nkb = (p.s + KB - 1) / KB;
  hipLaunchKernelGGL((bwd_kernel<SEG, true>), dim3(nkb, p.b * p.h), dim3(256), 0, st, p,
                     (const __bf16*)dout, (const float*)delta, dq_part, (__bf16*)dqkv);
  const int64_t n8 = (int64_t)p.b * p.s * p.h * D / 8;
  hipLaunchKernelGGL((dq_reduce_kernel<SEG, true>), dim3((unsigned)((n8 + 255) / 256)), dim3(256),
                     0, st, (const float*)dq_part, (__bf16*)dqkv, nkb, p.b, p.s, p.h,
                     p.scale_log2 / LOG2E, p.seg);
}

}  // namespace

void mv_attn_causal_fwd(const AttnParams& p, hipStream_t st) {
  if (p.seg) causal_fwd<true>(p, st);
  else causal_fwd<false>(p, st);
}

void mv_attn_causal_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                        float* dq_part, void* dqkv, hipStream_t st, float* bsum) {
  if (p.seg) causal_bwd<true>(p, out, dout, delta, dq_part, dqkv, st, bsum);
  else causal_bwd<false>(p, out, dout, delta, dq_part, dqkv, st, bsum);
}
