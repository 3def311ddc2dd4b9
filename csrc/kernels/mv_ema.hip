// mivod gfx950 kernels: the fp32 exponential moving average of the fp32 master weights on the
// flat-arena path (ema_decay of the mivod.optim.Fused* optimizers).
//
//   update     e[i] = e[i] + omd * (w[i] - e[i])      omd = fp32(1 - decay), rounded on the host
//              e[i] = w[i]                            where omd == 1.0f: the copying first update
//   swap       (w[i], e[i]) = (e[i], w[i]),  model[i] = cast(new w[i])
//   overwrite  w[i] = e[i],                  model[i] = cast(e[i])
//
// One streaming pass each: a workgroup per 4096-element chunk, 8 elements per lane through
// load8 / store8 where every stream of the launch is 16-byte aligned and the 8 are inside n,
// else one by one.  Both ways lead through the one unrolled instance of ema_one below (see
// mv_flat_step.h on why there is no second copy of the arithmetic).  The update reads 8 and
// writes 4 bytes per element.  Three roundings in the update (the difference, the product,
// the sum): the product goes through scaled(), so it is rounded to fp32 before the add and
// the result is that of three separate fp32 operations, which the CPU fallback reproduces
// bit for bit.  No atomics, nothing stored outside [0, n), nothing stored when *skip != 0.
#include "mv_ema.h"
#include "mv_common.h"

namespace mv {

enum EmaMode : int { kUpdate = 0, kSwap = 1, kOverwrite = 2 };

// one element: w and e in, w and e out
template <int MODE>
__device__ __forceinline__ void ema_one(float& w, float& e, float omd, bool copy) {
  if constexpr (MODE == kUpdate) {
    e = copy ? w : e + scaled(w - e, omd);
  } else if constexpr (MODE == kSwap) {
    const float t = w;
    w = e;
    e = t;
  } else {
    w = e;
  }
}

// update: w is read, e read and written, no model.  swap: both read and written.
// overwrite: e is read, w written.  model (nullable) receives cast(w) in swap and overwrite.
template <int MODE, typename TP>
__global__ __launch_bounds__(kBlock) void ema_kernel(float* __restrict__ w, float* __restrict__ e,
                                                      TP* __restrict__ model, int64_t n, float omd,
                                                      const int* __restrict__ skip) {
  if (skip && *skip) return;   // overflow guard: uniform, as the step kernels read it
  constexpr bool kLoadW = MODE != kOverwrite;
  constexpr bool kStoreW = MODE != kUpdate;
  constexpr bool kStoreE = MODE != kOverwrite;
  const bool copy = omd == 1.f;
  const bool vec = aligned16(w) && aligned16(e) && (!model || aligned16(model));
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  for (int64_t i = base + threadIdx.x * kVec; i < base + kChunk; i += kBlock * kVec) {
    const int cnt = (i + kVec <= n) ? kVec : (i < n ? (int)(n - i) : 0);
    if (cnt == 0) break;
    const bool full = vec && cnt == kVec;
    float wv[8], ev[8];
    if (full) {
      if constexpr (kLoadW) load8(w + i, wv);
      load8(e + i, ev);
    } else {
      for (int j = 0; j < kVec; ++j) {
        wv[j] = (kLoadW && j < cnt) ? w[i + j] : 0.f;
        ev[j] = j < cnt ? e[i + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) ema_one<MODE>(wv[j], ev[j], omd, copy);
    if (full) {
      if constexpr (kStoreW) store8(w + i, wv);
      if constexpr (kStoreE) store8(e + i, ev);
      if constexpr (kStoreW)
        if (model) store8(model + i, wv);
    } else {
      for (int j = 0; j < cnt; ++j) {
        if constexpr (kStoreW) w[i + j] = wv[j];
        if constexpr (kStoreE) e[i + j] = ev[j];
        if constexpr (kStoreW)
          if (model) st1(model + i + j, wv[j]);
      }
    }
  }
}

template <int MODE, typename TP>
static void launch_ema(float* w, float* e, void* model, int64_t n, float omd, const int* skip,
                       hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL((ema_kernel<MODE, TP>), dim3((unsigned)((n + kChunk - 1) / kChunk)),
                     dim3(kBlock), 0, st, w, e, reinterpret_cast<TP*>(model), n, omd, skip);
}

template <int MODE>
static void launch_ema_model(float* w, float* e, void* model, int md, int64_t n, const int* skip,
                             hipStream_t st) {
  if (!model) md = F32;   // a null model stream: the instantiation does not matter
  switch (md) {
    case F32: launch_ema<MODE, float>(w, e, model, n, 0.f, skip, st); break;
    case BF16: launch_ema<MODE, __bf16>(w, e, model, n, 0.f, skip, st); break;
    case F16: launch_ema<MODE, _Float16>(w, e, model, n, 0.f, skip, st); break;
  }
}

}  // namespace mv

using namespace mv;

void mv_launch_ema_update(const float* w, float* e, int64_t n, float omd, const int* skip,
                          hipStream_t st) {
  // the update mode only reads w
  launch_ema<kUpdate, float>(const_cast<float*>(w), e, nullptr, n, omd, skip, st);
}

void mv_launch_ema_swap(float* w, float* e, void* model, int model_dtype, int64_t n,
                        const int* skip, hipStream_t st) {
  launch_ema_model<kSwap>(w, e, model, model_dtype, n, skip, st);
}

void mv_launch_ema_overwrite(float* w, const float* e, void* model, int model_dtype, int64_t n,
                             const int* skip, hipStream_t st) {
  // the overwrite mode only reads e
  launch_ema_model<kOverwrite>(w, const_cast<float*>(e), model, model_dtype, n, skip, st);
}
