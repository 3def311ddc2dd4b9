// mivod gfx950 kernels: the streaming skeleton of the fused elementwise optimizer steps on
// flat buckets (K6: SGD, Adam and Adadelta in mv_kernels.hip, Adagrad in mv_adaptive.hip) and
// the (gradient dtype x model dtype) dispatch of all the K6 launchers.  Included only by the
// .hip files, never by the bindings.
#pragma once
#include "mv_common.h"

#include <utility>

namespace mv {

// gscale under the nullable device clip coefficient of global gradient-norm clipping
// (mv_clip.hip): one fp32 product, taken once per thread before the element loop, so a
// clipped launch is the unclipped launch of gscale * gclip[0] bit for bit.  The product is
// uniform and goes back into a scalar register, where the element loop found gscale before
// the operand existed: left in a vector register it cost every instantiation two VGPRs
// (rmsprop_flat_kernel reached 80, the edge of its occupancy step).  Either way the operand
// moves registers around, which is enough to change the product that -ffp-contract=fast fuses
// in an a*b + c*d (sgd_flat_kernel spells its one out for that reason).
__device__ __forceinline__ float clipped_gscale(float gscale, const float* __restrict__ gclip) {
  if (!gclip) return gscale;
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(gscale * *gclip)));
}

// f(g, w, s0, .., s{NS-1}) on element j of the registers.  The state reaches f as NS references
// into sv, not as a float (&)[NS] gathered from it and scattered back: the copies change the
// register allocation (RMSprop's arithmetic on this loop: 104-114 VGPRs with them, 72-84
// without).
template <typename F, size_t... K>
__device__ __forceinline__ void flat_step_apply(F& f, float g, float& w, float (&sv)[sizeof...(K)][8],
                                                int j, std::index_sequence<K...>) {
  f(g, w, sv[K][j]...);
}

// The chunk of workgroup blockIdx.x in a launch of MV_GRID(n) workgroups of kBlock lanes
// over [0, n): the gradient read once in the wire dtype (TG), the fp32 master and NS fp32
// state streams read and written once, the low-precision model copy (TP) written in the same
// pass.  A null st[k] or model is a stream this launch does not have: it is neither loaded
// nor stored, and f tests the same pointer before it uses that reference.
//
// A lane takes kVec consecutive elements per step: through load8 / store8 where all of them
// are inside n and every stream is 16-byte aligned (chunks start at multiples of 4096
// elements, so the bases decide it for the whole launch), else one by one, padded with zeros
// past n (every element of an offset view goes this way).  Both ways lead through the ONE
// unrolled instance of f below, the only place the optimizer's arithmetic exists; that is
// what makes a result independent of n % kVec and of the alignment.  -ffp-contract=fast
// fuses a*b + c*d differently in a second inlined copy of the same expression (in a
// lane-per-element tail loop, SGD's momentum update became one fma where the vector body
// rounds both products), so there must not be a second copy.
//
// The null tests cost registers and move the compiler's choice of which product of a*b + c*d
// to fuse, so a kernel whose streams are all required says so with __builtin_assume (Adam's
// m update and Adadelta's 59 VGPRs depend on it); its launcher's declaration names the contract.
//
// Not on this: lars_flat_kernel, whose vector body and tail loop are such two copies and do
// round differently, so no single copy gives the bits of both; rmsprop_flat_kernel, whose
// register allocation crosses an occupancy step on it (79 -> 82 VGPRs and more, 6 -> 5 waves
// per SIMD, with the assume or without); lamb_moments_kernel, which reduces per lane and
// never writes w; lamb_apply_kernel, which reads no gradient and writes back no state.
template <int NS, typename TG, typename TP, typename F>
__device__ __forceinline__ void flat_step(const TG* __restrict__ g, float* __restrict__ w,
                                          float* const (&st)[NS], TP* __restrict__ model,
                                          int64_t n, F f) {
  bool vec = aligned16(g) && aligned16(w) && (!model || aligned16(model));
#pragma unroll
  for (int k = 0; k < NS; ++k) vec = vec && (!st[k] || aligned16(st[k]));
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  for (int64_t i = base + threadIdx.x * kVec; i < base + kChunk; i += kBlock * kVec) {
    const int cnt = (i + kVec <= n) ? kVec : (i < n ? (int)(n - i) : 0);
    if (cnt == 0) break;
    const bool full = vec && cnt == kVec;
    float gv[8], wv[8], sv[NS][8];
    if (full) {
      load8(g + i, gv);
      load8(w + i, wv);
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (st[k]) load8(st[k] + i, sv[k]);
    } else {
      for (int j = 0; j < kVec; ++j) {
        gv[j] = j < cnt ? ld1(g + i + j) : 0.f;
        wv[j] = j < cnt ? w[i + j] : 0.f;
#pragma unroll
        for (int k = 0; k < NS; ++k) sv[k][j] = (st[k] && j < cnt) ? st[k][i + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      flat_step_apply(f, gv[j], wv[j], sv, j, std::make_index_sequence<NS>());
    if (full) {
      store8(w + i, wv);
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (st[k]) store8(st[k] + i, sv[k]);
      if (model) store8(model + i, wv);
    } else {
      for (int j = 0; j < cnt; ++j) {
        w[i + j] = wv[j];
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (st[k]) st[k][i + j] = sv[k][j];
        if (model) st1(model + i + j, wv[j]);
      }
    }
  }
}

}  // namespace mv

// ---- host side: the launch grid over n elements and the TG x TP instantiation ----
#define MV_GRID(n) dim3((unsigned)(((n) + kChunk - 1) / kChunk))

#define DISPATCH_GP(gd, md, MACRO)                                  \
  do {                                                              \
    if (md == F32) {                                                \
      using TP = float;                                             \
      if (gd == F32) { using TG = float; MACRO; }                   \
      else if (gd == BF16) { using TG = __bf16; MACRO; }            \
      else { using TG = _Float16; MACRO; }                          \
    } else if (md == BF16) {                                        \
      using TP = __bf16;                                            \
      if (gd == F32) { using TG = float; MACRO; }                   \
      else if (gd == BF16) { using TG = __bf16; MACRO; }            \
      else { using TG = _Float16; MACRO; }                          \
    } else {                                                        \
      using TP = _Float16;                                          \
      if (gd == F32) { using TG = float; MACRO; }                   \
      else if (gd == BF16) { using TG = __bf16; MACRO; }            \
      else { using TG = _Float16; MACRO; }                          \
    }                                                               \
  } while (0)
