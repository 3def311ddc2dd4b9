// mivod gfx950 kernels: local gradient accumulation in an fp32 flat arena
// (DistributedOptimizer(backward_passes_per_step=k, accumulation_dtype=torch.float32)).
//
// One multi-tensor launch per bucket per micro-pass replaces autograd's per-parameter
// p.grad += g in the parameter's own dtype:
//
//   first  acc[off + i]  = float(g[i])          pass 1 of a window (a write: no zeroing pass)
//   add    acc[off + i] += float(g[i])          passes 2 .. k-1
//   last   dst[off + i]  = cast_W((acc[off + i] + float(g[i])) * scale)
//                                               pass k, fused with the wire cast of the pack;
//                                               acc is not written (the next window's first
//                                               pass overwrites it)
//
// The conversions to fp32 are exact, so over k passes a wire value carries k-1 fp32 additions,
// the rounding of scale to fp32, one multiply and the cast.  All three stream every byte once:
// the tensor table travels in the kernel arguments as in mt_copy_kernel (MtArgs, uniform
// binary search over chunk_start), one workgroup per 4096-element chunk, 8 elements per lane
// through load8 / store8 when every pointer of the chunk is 16-byte aligned, one by one
// otherwise and for the tail.  No atomics but the flag's atomicOr.
#include "mv_accum.h"
#include "mv_common.h"

namespace mv {

enum AccumMode : int { kFirst = 0, kAdd = 1, kLast = 2 };

// one element: the accumulator's new value (first, add) or the wire value (last)
template <int MODE>
__device__ __forceinline__ float accum_one(float a, float g, float scale) {
  if constexpr (MODE == kFirst) return g;
  else if constexpr (MODE == kAdd) return a + g;
  else return scaled(a + g, scale);
}

// T: gradient dtype, W: wire dtype (float for first / add, where dst is unused).
// acc is read (add, last) or written (first, add); it never aliases g or dst.
template <typename T, typename W, int MODE>
__global__ __launch_bounds__(kBlock) void accum_kernel(MtArgs args, float* __restrict__ acc,
                                                        W* __restrict__ dst, float scale,
                                                        int* found_nonfinite) {
  const int b = blockIdx.x;
  // uniform binary search: largest t with chunk_start[t] <= b
  int lo = 0, hi = args.ntensors - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (args.chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const int t = lo;
  const int64_t begin = (int64_t)(b - args.chunk_start[t]) * kChunk;
  const int64_t numel = args.numel[t];
  const int64_t n = (numel - begin < kChunk) ? (numel - begin) : kChunk;
  if (n <= 0) return;
  const T* __restrict__ g = reinterpret_cast<const T*>(args.ptr[t]) + begin;
  float* __restrict__ a = acc + args.flat_off[t] + begin;
  W* __restrict__ d = nullptr;
  if constexpr (MODE == kLast) d = dst + args.flat_off[t] + begin;
  bool bad = false;
  const bool vec = aligned16(g) && aligned16(a) && (MODE != kLast || aligned16(d));
  const int64_t nv = vec ? n / kVec : 0;
  for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
    float gv[8], av[8];
    load8(g + i * kVec, gv);
    if constexpr (MODE != kFirst) load8(a + i * kVec, av);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      av[j] = accum_one<MODE>(MODE == kFirst ? 0.f : av[j], gv[j], scale);
      if constexpr (MODE == kLast)
        if (found_nonfinite) bad |= !__builtin_isfinite(stored<W>(av[j]));
    }
    if constexpr (MODE == kLast) store8(d + i * kVec, av);
    else store8(a + i * kVec, av);
  }
  for (int64_t i = nv * kVec + threadIdx.x; i < n; i += kBlock) {
    const float x = accum_one<MODE>(MODE == kFirst ? 0.f : a[i], ld1(g + i), scale);
    if constexpr (MODE == kLast) {
      if (found_nonfinite) bad |= !__builtin_isfinite(stored<W>(x));
      st1(d + i, x);
    } else {
      a[i] = x;
    }
  }
  if constexpr (MODE == kLast)
    if (found_nonfinite && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(found_nonfinite, 1);
}

template <typename T, typename W, int MODE>
static void launch_accum(const MtArgs& a, float* acc, void* dst, float scale, int* nf,
                         hipStream_t st) {
  const int nblocks = a.chunk_start[a.ntensors];
  if (nblocks <= 0) return;
  hipLaunchKernelGGL((accum_kernel<T, W, MODE>), dim3(nblocks), dim3(kBlock), 0, st, a, acc,
                     reinterpret_cast<W*>(dst), scale, nf);
}

template <typename T>
static void launch_last(const MtArgs& a, float* acc, void* dst, int wd, float scale, int* nf,
                        hipStream_t st) {
  switch (wd) {
    case F32: launch_accum<T, float, kLast>(a, acc, dst, scale, nf, st); break;
    case BF16: launch_accum<T, __bf16, kLast>(a, acc, dst, scale, nf, st); break;
    case F16: launch_accum<T, _Float16, kLast>(a, acc, dst, scale, nf, st); break;
  }
}

template <typename T>
static void launch_into(const MtArgs& a, float* acc, bool first, hipStream_t st) {
  if (first) launch_accum<T, float, kFirst>(a, acc, nullptr, 1.f, nullptr, st);
  else launch_accum<T, float, kAdd>(a, acc, nullptr, 1.f, nullptr, st);
}

}  // namespace mv

using namespace mv;

void mv_launch_accumulate(const MtArgs& a, int grad_dtype, float* acc, bool first,
                          hipStream_t st) {
  switch (grad_dtype) {
    case F32: launch_into<float>(a, acc, first, st); break;
    case BF16: launch_into<__bf16>(a, acc, first, st); break;
    case F16: launch_into<_Float16>(a, acc, first, st); break;
  }
}

void mv_launch_pack_accumulated(const MtArgs& a, int grad_dtype, const float* acc, void* dst,
                                int wire_dtype, float scale, int* found_nonfinite,
                                hipStream_t st) {
  float* ap = const_cast<float*>(acc);      // the last mode only reads it
  switch (grad_dtype) {
    case F32: launch_last<float>(a, ap, dst, wire_dtype, scale, found_nonfinite, st); break;
    case BF16: launch_last<__bf16>(a, ap, dst, wire_dtype, scale, found_nonfinite, st); break;
    case F16: launch_last<_Float16>(a, ap, dst, wire_dtype, scale, found_nonfinite, st); break;
  }
}
