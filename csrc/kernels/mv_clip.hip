// mivod gfx950 kernels: global gradient-norm clipping on the flat-bucket path (max_grad_norm
// of the mivod.optim.Fused* optimizers).
//
//   grad_sumsq_kernel     one read-only streaming pass over a REDUCED bucket in the wire dtype:
//                         one fp32 sum of squares per 4096-element chunk, and (optionally) the
//                         overflow guard's non-finite flag from the same loads
//   clip_finalize_kernel  the partials of every bucket of the step -> the clip coefficient
//                         min(1, max_norm / (norm + 1e-6)) and the norm, on the device
//   the K6 step kernels (mv_kernels.hip, mv_adaptive.hip) multiply their gscale by the
//   coefficient they read through the nullable gclip pointer.
//
// Every rank holds the same reduced bits, and every add below happens in an order fixed by
// the element index alone (no float atomics, nothing that depends on scheduling), so every
// rank derives the same coefficient without a collective or a host round trip.
#include "mv_clip.h"
#include "mv_common.h"

namespace mv {

// Workgroup b covers x[b*kChunk, (b+1)*kChunk) clipped to n, with the element -> lane mapping
// of flat_step (mv_flat_step.h): lane t takes the kVec consecutive elements from
// t*kVec + s*kBlock*kVec in step s, through load8 where the base is 16-byte aligned and all
// of them are inside n, else one by one with zeros past n.  The sum order is therefore the
// same on both paths: element 0..7 of step 0, then of step 1, in the lane; the wave butterfly;
// the four waves in order.  Adding the zeros of the padding is exact.
template <typename T>
__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(const T* __restrict__ x, int64_t n,
                                                             float* __restrict__ partial,
                                                             int* __restrict__ flag) {
  const bool vec = aligned16(x);
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  float acc[1] = {0.f};
  bool bad = false;
#pragma unroll
  for (int s = 0; s < kChunk / (kBlock * kVec); ++s) {
    const int64_t i = base + (int64_t)(s * kBlock + threadIdx.x) * kVec;
    const int cnt = (i + kVec <= n) ? kVec : (i < n ? (int)(n - i) : 0);
    float v[8];
    if (vec && cnt == kVec) {
      load8(x + i, v);
    } else {
      for (int j = 0; j < kVec; ++j) v[j] = j < cnt ? ld1(x + i + j) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[0] += v[j] * v[j];
      bad |= !__builtin_isfinite(v[j]);
    }
  }
  block_sum<1>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
  if (flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// One workgroup.  Lane t adds partial[t], partial[t + 256], .. in float64, then a binary tree
// over the 256 lanes in LDS: a fixed order.  The float64 roundings (at most total/256 + 8 adds,
// a root, a product, an add and a quotient, 2^-53 each) vanish next to the one fp32 rounding
// of each stored result.
__global__ __launch_bounds__(kBlock) void clip_finalize_kernel(const float* __restrict__ partial,
                                                                int64_t total, double gscale,
                                                                double max_norm,
                                                                float* __restrict__ clip) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += kBlock) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = red[0];
    const double norm = gscale * sqrt(sum);
    const double q = max_norm / (norm + 1e-6);
    double coef = q > 1.0 ? 1.0 : q;
    // a non-finite norm must not clip to a finite coefficient (max_norm / inf is 0, which
    // would silently zero the gradient): the update it scales goes non-finite instead, and
    // with the overflow guard on the step is skipped anyway
    if (!__builtin_isfinite(sum)) coef = __builtin_nan("");
    clip[0] = (float)coef;
    clip[1] = (float)norm;
  }
}

}  // namespace mv

using namespace mv;

void mv_launch_grad_sumsq(const void* x, int dt, int64_t n, float* partial, int* flag,
                          hipStream_t st) {
  const int nb = (int)((n + kChunk - 1) / kChunk);
  if (nb <= 0) return;
  switch (dt) {
    case F32: hipLaunchKernelGGL((grad_sumsq_kernel<float>), dim3(nb), dim3(kBlock), 0, st, (const float*)x, n, partial, flag); break;
    case BF16: hipLaunchKernelGGL((grad_sumsq_kernel<__bf16>), dim3(nb), dim3(kBlock), 0, st, (const __bf16*)x, n, partial, flag); break;
    case F16: hipLaunchKernelGGL((grad_sumsq_kernel<_Float16>), dim3(nb), dim3(kBlock), 0, st, (const _Float16*)x, n, partial, flag); break;
  }
}

void mv_launch_clip_finalize(const float* partial, int64_t total, double gscale, double max_norm,
                             float* clip, hipStream_t st) {
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partial,
                     total < 0 ? 0 : total, gscale, max_norm, clip);
}
