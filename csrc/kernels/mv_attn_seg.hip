// Block-diagonal attention for packed sequences: the segmented instantiations (SEG = true)
// of the kernel templates in mv_attn_kernels.h, their launchers, and the prep kernel that
// turns segment ids into per-token run bounds.  docs/PACKED_ATTENTION.md has the contract.
#include "mv_attn_kernels.h"

namespace mv {
namespace attn {

// ids [b, s] -> bounds [b, s]: token t's maximal run of equal ids [lo, hi) as lo | hi << 16,
// 0 (lo == hi) for a negative id.  One 256-thread workgroup per batch row, two chunked
// scans with a carry: lo = the running max of the run starts at or before t (left to
// right), hi = the running min of the run ends after t (right to left).  Wave scans by
// lane shifts (max / min are idempotent: a lane whose source is out of range reads itself),
// wave totals through LDS.  No host sync, no atomics; the attention kernels only read.
template <typename T>
__global__ __launch_bounds__(256) void seg_bounds_kernel(const T* __restrict__ ids,
                                                          uint32_t* __restrict__ bounds, int s) {
  const T* row = ids + (int64_t)blockIdx.x * s;
  uint32_t* out = bounds + (int64_t)blockIdx.x * s;
  __shared__ int tot[4];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int nch = (s + 255) / 256;
  int carry = 0;                                     // token 0 starts a run
  for (int ch = 0; ch < nch; ++ch) {
    const int t = ch * 256 + tid;
    int v = -1;
    if (t < s && (t == 0 || row[t] != row[t - 1])) v = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_up(v, d, 64));
    if (l == 63) tot[w] = v;
    __syncthreads();
    int pre = carry;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < w) pre = max(pre, tot[i]);
      carry = max(carry, tot[i]);
    }
    if (t < s) out[t] = (uint32_t)max(v, pre);
    __syncthreads();
  }
  carry = s;                                         // token s - 1 ends a run
  for (int ch = nch - 1; ch >= 0; --ch) {
    const int t = ch * 256 + tid;
    int v = INT_MAX;
    if (t < s && (t == s - 1 || row[t + 1] != row[t])) v = t + 1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = min(v, __shfl_down(v, d, 64));
    if (l == 0) tot[w] = v;
    __syncthreads();
    int pre = carry;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i > w) pre = min(pre, tot[i]);
      carry = min(carry, tot[i]);
    }
    // out[t] holds this thread's own lo from the first scan
    if (t < s) out[t] = row[t] >= 0 ? (out[t] | ((uint32_t)min(v, pre) << 16)) : 0u;
    __syncthreads();
  }
}

}  // namespace attn
}  // namespace mv

using namespace mv::attn;

void mv_attn_seg_bounds(const void* ids, bool ids64, uint32_t* bounds, int b, int s,
                        hipStream_t st) {
  if (ids64)
    hipLaunchKernelGGL(seg_bounds_kernel<int64_t>, dim3(b), dim3(256), 0, st,
                       (const int64_t*)ids, bounds, s);
  else
    hipLaunchKernelGGL(seg_bounds_kernel<int32_t>, dim3(b), dim3(256), 0, st,
                       (const int32_t*)ids, bounds, s);
}

void mv_attn_seg_fwd(const AttnParams& p, hipStream_t st) {
  if (p.s <= 2 * KB) {
    hipLaunchKernelGGL((fwd_short_kernel<6, true>), dim3(p.b * p.h), dim3(512), 0, st, p);
    return;
  }
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h);
  hipLaunchKernelGGL(fwd_kernel<true>, grid, dim3(256), 0, st, p);
}

void mv_attn_seg_bwd(const AttnParams& p, const void* out, const void* dout, const float* delta,
                     float* dq_part, void* dqkv, hipStream_t st, float* bsum) {
  if (p.s <= 2 * KB) {
    hipLaunchKernelGGL(bwd_short_kernel<true>, dim3(p.b * p.h), dim3(512), 0, st, p,
                       (const __bf16*)out, (const __bf16*)dout, (__bf16*)dqkv, bsum);
    return;
  }
  const int nkb = (p.s + KB - 1) / KB;
  hipLaunchKernelGGL(bwd_kernel<true>, dim3(nkb, p.b * p.h), dim3(256), 0, st, p,
                     (const __bf16*)dout, delta, dq_part, (__bf16*)dqkv);
  const int64_t n8 = (int64_t)p.b * p.s * p.h * D / 8;
  hipLaunchKernelGGL(dq_reduce_kernel<true>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0,
                     st, (const float*)dq_part, (__bf16*)dqkv, nkb, p.b, p.s, p.h,
                     p.scale_log2 / LOG2E, p.seg);
}
