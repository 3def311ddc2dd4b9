// mivod gfx950 kernels: RMSprop and Adagrad on flat buckets (K6, next to mv_kernels.hip's
// SGD / Adam / Adadelta).  Pure streaming updates: one workgroup of 256 lanes per 4096-element
// chunk, 8 elements per lane per step through load8 / store8 (16-byte accesses), a scalar tail
// for the last n % 8 elements, the gradient read once in the wire dtype (TG), fp32 master and
// state read and written once, the optional low-precision model copy (TP) written in the same
// pass.  Adagrad is its arithmetic on mv_flat_step.h's skeleton; RMSprop is the same loop
// written out (that header says why).  Both guard their vector body: when any base pointer
// is not 16-byte aligned (an offset view; the arenas never produce one) every element goes
// through the scalar path, uniformly over the launch.
//
// Bytes per element with an fp16 wire and a bf16 model: g 2 + w 4+4 + model 2 = 12, plus 8 per
// state buffer: 20 (plain RMSprop, Adagrad), 28 (momentum or centered), 36 (both).
#include "mv_adaptive.h"
#include "mv_flat_step.h"

using namespace mv;

namespace mv {

// oma = 1 - alpha, taken on the host in double and rounded once (mv_kernels.hip, at SgdHp)
struct RmspropHp { float lr, alpha, oma, eps, wd, gscale, momentum; };
struct AdagradHp { float lr, eps, wd, gscale; };

__device__ __forceinline__ bool aligned16_or_null(const void* p) { return !p || aligned16(p); }

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void rmsprop_flat_kernel(const TG* __restrict__ g,
                                                               float* __restrict__ w,
                                                               float* __restrict__ sq,
                                                               float* __restrict__ ga,
                                                               float* __restrict__ buf,
                                                               TP* __restrict__ model, int64_t n,
                                                               RmspropHp hp,
                                                               const float* __restrict__ dyn,
                                                               const int* __restrict__ skip,
                                                               const float* __restrict__ gclip) {
  if (skip && *skip) return;   // overflow guard: every rank skips this step identically
  hp.gscale = clipped_gscale(hp.gscale, gclip);   // global-norm clip coefficient (mv_clip.hip)
  if (dyn) hp.lr = dyn[0];
  const bool vec = aligned16(g) && aligned16(w) && aligned16(sq) && aligned16_or_null(ga) &&
                   aligned16_or_null(buf) && aligned16_or_null(model);
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  for (int64_t i = base + threadIdx.x * kVec; i < base + kChunk; i += kBlock * kVec) {
    const int cnt = (i + kVec <= n) ? kVec : (i < n ? (int)(n - i) : 0);
    if (cnt == 0) break;
    const bool full = vec && cnt == kVec;
    float gv[8], wv[8], sv[8], av[8], bv[8];
    if (full) {
      load8(g + i, gv); load8(w + i, wv); load8(sq + i, sv);
      if (ga) load8(ga + i, av);
      if (buf) load8(buf + i, bv);
    } else {
      for (int j = 0; j < kVec; ++j) {
        gv[j] = j < cnt ? ld1(g + i + j) : 0.f; wv[j] = j < cnt ? w[i + j] : 0.f;
        sv[j] = j < cnt ? sq[i + j] : 0.f;
        av[j] = (ga && j < cnt) ? ga[i + j] : 0.f;
        bv[j] = (buf && j < cnt) ? buf[i + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gr = gv[j] * hp.gscale + hp.wd * wv[j];
      sv[j] = hp.alpha * sv[j] + hp.oma * gr * gr;
      float x = sv[j];
      if (ga) {
        av[j] = hp.alpha * av[j] + hp.oma * gr;
        // sq - ga^2 >= 0 in exact arithmetic; rounded, it can fall below zero (torch takes the
        // root of it as it is and gets NaN)
        x = fmaxf(sv[j] - av[j] * av[j], 0.f);
      }
      float q = gr / (sqrtf(x) + hp.eps);
      if (buf) {
        bv[j] = hp.momentum * bv[j] + q;
        q = bv[j];
      }
      wv[j] -= hp.lr * q;
    }
    if (full) {
      store8(w + i, wv); store8(sq + i, sv);
      if (ga) store8(ga + i, av);
      if (buf) store8(buf + i, bv);
      if (model) store8(model + i, wv);
    } else {
      for (int j = 0; j < cnt; ++j) {
        w[i + j] = wv[j]; sq[i + j] = sv[j];
        if (ga) ga[i + j] = av[j];
        if (buf) buf[i + j] = bv[j];
        if (model) st1(model + i + j, wv[j]);
      }
    }
  }
}

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void adagrad_flat_kernel(const TG* __restrict__ g,
                                                               float* __restrict__ w,
                                                               float* __restrict__ sum,
                                                               TP* __restrict__ model, int64_t n,
                                                               AdagradHp hp,
                                                               const float* __restrict__ dyn,
                                                               const int* __restrict__ skip,
                                                               const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) hp.lr = dyn[0];
  __builtin_assume(sum != nullptr);   // always given: drops flat_step's null tests, as in Adam
  float* const st[1] = {sum};
  flat_step<1>(g, w, st, model, n, [&](float gj, float& wj, float& sj) {
    const float gr = gj * hp.gscale + hp.wd * wj;
    sj += gr * gr;
    wj -= hp.lr * (gr / (sqrtf(sj) + hp.eps));
  });
}

}  // namespace mv

// ---------------- host launchers (MV_GRID, DISPATCH_GP: mv_flat_step.h) ----------------
void mv_launch_rmsprop(const void* g, int gd, float* w, float* sq, float* ga, float* buf,
                       void* model, int md, int64_t n, float lr, double alpha, float eps, float wd,
                       float momentum, float gscale, const float* dyn, const int* skip,
                       const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  RmspropHp hp{lr, (float)alpha, (float)(1.0 - alpha), eps, wd, gscale, momentum};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((rmsprop_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, sq, ga, buf, (TP*)model, n, hp, dyn,
                                         skip, gclip));
}

void mv_launch_adagrad(const void* g, int gd, float* w, float* sum, void* model, int md, int64_t n,
                       float lr, float eps, float wd, float gscale, const float* dyn,
                       const int* skip, const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  AdagradHp hp{lr, eps, wd, gscale};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((adagrad_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, sum, (TP*)model, n, hp, dyn, skip,
                                         gclip));
}
