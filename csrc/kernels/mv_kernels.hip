// mivod hand-written CDNA4 (gfx950) kernels for the data-parallel gradient path.
//
// Replaces, MI355X-first, what the reference's engine (horovod 0.18.1, used by
// /root/reference/mnist_keras.py:87 and tensorflow2_keras_mnist.py:58) does with
// per-tensor cudaMemcpyAsync + TF elementwise ops + NCCL-side scaling:
//   K1/K2  mv_mt_copy        multi-tensor fusion-buffer pack / unpack, fused cast
//                            (fp32/bf16/fp16 compression) and pre/post scale
//   K4/K5  mv_flat_cast      flat compress / decompress / scale of a bucket
//   K6     mv_{sgd,adam,adadelta}_flat, mv_lars_*, mv_lamb_*  fused optimizer steps that
//                            run directly on a reduced flat gradient bucket,
//                            fp32 master weights + bf16 model copy written in
//                            the same pass (grad read once); SGD, Adam and Adadelta
//                            on the streaming skeleton of mv_flat_step.h
//   K8     mv_seg_dot3 / mv_adasum_combine  Adasum per-tensor Gram terms and
//                            the (1-d/2|a|^2)a + (1-d/2|b|^2)b merge
// See SURVEY.md §2.5.b for the inventory.  All kernels are HBM-bound: the design
// goal is 16-byte lanes, >=1k workgroups per launch and a single pass over
// every byte (no separate scale / cast / unscale passes).
#include "mv_common.h"
#include "mv_flat_step.h"
#include "mv_kernels.h"

namespace mv {

// -------------------------------------------------------------------------
// K1/K2: multi-tensor pack / unpack.
// The tensor table travels in the kernel arguments (no H2D copy, graph-capture
// safe).  Workgroup b finds its tensor by a uniform binary search over the
// chunk prefix sums (scalar loads from the kernarg segment).
// -------------------------------------------------------------------------
template <typename TS, typename TD>
__device__ __forceinline__ void copy_range(const TS* __restrict__ s, TD* __restrict__ d,
                                           int64_t n, float scale, int* found_nonfinite) {
  bool bad = false;
  if (aligned16(s) && aligned16(d)) {
    const int64_t nv = n / kVec;
    for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
      float v[8];
      load8(s + i * kVec, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = scaled(v[j], scale);
        if (found_nonfinite) bad |= !__builtin_isfinite(stored<TD>(v[j]));
      }
      store8(d + i * kVec, v);
    }
    for (int64_t i = nv * kVec + threadIdx.x; i < n; i += kBlock) {
      float x = scaled(ld1(s + i), scale);
      if (found_nonfinite) bad |= !__builtin_isfinite(stored<TD>(x));
      st1(d + i, x);
    }
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
      float x = scaled(ld1(s + i), scale);
      if (found_nonfinite) bad |= !__builtin_isfinite(stored<TD>(x));
      st1(d + i, x);
    }
  }
  if (found_nonfinite && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(found_nonfinite, 1);
}

template <typename TT, typename TF, bool TO_FLAT>
__global__ __launch_bounds__(kBlock) void mt_copy_kernel(MtArgs args, TF* __restrict__ flat,
                                                          float scale, int* found_nonfinite) {
  const int b = blockIdx.x;
  // uniform binary search: largest t with chunk_start[t] <= b
  int lo = 0, hi = args.ntensors - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (args.chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const int t = lo;
  const int64_t c = b - args.chunk_start[t];
  const int64_t begin = c * kChunk;
  const int64_t numel = args.numel[t];
  const int64_t n = (numel - begin < kChunk) ? (numel - begin) : kChunk;
  if (n <= 0) return;
  TT* tp = reinterpret_cast<TT*>(args.ptr[t]) + begin;
  TF* fp = flat + args.flat_off[t] + begin;
  if constexpr (TO_FLAT) copy_range<TT, TF>(tp, fp, n, scale, found_nonfinite);
  else copy_range<TF, TT>(fp, tp, n, scale, found_nonfinite);
}

template <typename TT, typename TF>
static void launch_mt(const MtArgs& a, void* flat, bool to_flat, float scale, int* nf,
                      hipStream_t st) {
  const int nblocks = a.chunk_start[a.ntensors];
  if (nblocks <= 0) return;
  if (to_flat)
    hipLaunchKernelGGL((mt_copy_kernel<TT, TF, true>), dim3(nblocks), dim3(kBlock), 0, st, a,
                       reinterpret_cast<TF*>(flat), scale, nf);
  else
    hipLaunchKernelGGL((mt_copy_kernel<TT, TF, false>), dim3(nblocks), dim3(kBlock), 0, st, a,
                       reinterpret_cast<TF*>(flat), scale, nf);
}

template <typename TT>
static void dispatch_flat(const MtArgs& a, void* flat, int flat_dtype, bool to_flat, float scale,
                          int* nf, hipStream_t st) {
  switch (flat_dtype) {
    case F32: launch_mt<TT, float>(a, flat, to_flat, scale, nf, st); break;
    case BF16: launch_mt<TT, __bf16>(a, flat, to_flat, scale, nf, st); break;
    case F16: launch_mt<TT, _Float16>(a, flat, to_flat, scale, nf, st); break;
  }
}

}  // namespace mv

using namespace mv;

void mv_launch_mt_copy(const MtArgs& a, int tensor_dtype, void* flat, int flat_dtype,
                       bool to_flat, float scale, int* found_nonfinite, hipStream_t st) {
  switch (tensor_dtype) {
    case F32: dispatch_flat<float>(a, flat, flat_dtype, to_flat, scale, found_nonfinite, st); break;
    case BF16: dispatch_flat<__bf16>(a, flat, flat_dtype, to_flat, scale, found_nonfinite, st); break;
    case F16: dispatch_flat<_Float16>(a, flat, flat_dtype, to_flat, scale, found_nonfinite, st); break;
  }
}

// -------------------------------------------------------------------------
// K4/K5: flat cast + scale (compress / decompress / average in place)
// -------------------------------------------------------------------------
namespace mv {
template <typename TS, typename TD>
__global__ __launch_bounds__(kBlock) void flat_cast_kernel(const TS* __restrict__ s,
                                                            TD* __restrict__ d, int64_t n,
                                                            float scale, int* nf) {
  const int64_t begin = (int64_t)blockIdx.x * kChunk;
  const int64_t cnt = (n - begin < kChunk) ? (n - begin) : kChunk;
  copy_range<TS, TD>(s + begin, d + begin, cnt, scale, nf);
}
template <typename TS>
static void flat_cast_d(const void* s, void* d, int dd, int64_t n, float scale, int* nf,
                        hipStream_t st) {
  const int nb = (int)((n + kChunk - 1) / kChunk);
  if (nb <= 0) return;
  const TS* sp = reinterpret_cast<const TS*>(s);
  switch (dd) {
    case F32: hipLaunchKernelGGL((flat_cast_kernel<TS, float>), dim3(nb), dim3(kBlock), 0, st, sp, (float*)d, n, scale, nf); break;
    case BF16: hipLaunchKernelGGL((flat_cast_kernel<TS, __bf16>), dim3(nb), dim3(kBlock), 0, st, sp, (__bf16*)d, n, scale, nf); break;
    case F16: hipLaunchKernelGGL((flat_cast_kernel<TS, _Float16>), dim3(nb), dim3(kBlock), 0, st, sp, (_Float16*)d, n, scale, nf); break;
  }
}
}  // namespace mv

void mv_launch_flat_cast(const void* src, int sd, void* dst, int dd, int64_t n, float scale,
                         int* found_nonfinite, hipStream_t st) {
  switch (sd) {
    case F32: flat_cast_d<float>(src, dst, dd, n, scale, found_nonfinite, st); break;
    case BF16: flat_cast_d<__bf16>(src, dst, dd, n, scale, found_nonfinite, st); break;
    case F16: flat_cast_d<_Float16>(src, dst, dd, n, scale, found_nonfinite, st); break;
  }
}

// -------------------------------------------------------------------------
// Overflow guard: read-only non-finite scan of a REDUCED bucket.  A non-finite
// contribution of any rank (or an overflow inside the reduction) propagates
// into the reduced sum, and every rank holds the same reduced bits, so every
// rank sets the same flag without another collective.
// -------------------------------------------------------------------------
namespace mv {
template <typename T>
__global__ __launch_bounds__(kBlock) void nonfinite_scan_kernel(const T* __restrict__ x, int64_t n,
                                                                 int* __restrict__ flag) {
  const int64_t begin = (int64_t)blockIdx.x * kChunk;
  const int64_t cnt = (n - begin < kChunk) ? (n - begin) : kChunk;
  const T* s = x + begin;
  bool bad = false;
  if (aligned16(s)) {
    const int64_t nv = cnt / kVec;
    for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
      float v[8];
      load8(s + i * kVec, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) bad |= !__builtin_isfinite(v[j]);
    }
    for (int64_t i = nv * kVec + threadIdx.x; i < cnt; i += kBlock) bad |= !__builtin_isfinite(ld1(s + i));
  } else {
    for (int64_t i = threadIdx.x; i < cnt; i += kBlock) bad |= !__builtin_isfinite(ld1(s + i));
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
}  // namespace mv

void mv_launch_nonfinite_scan(const void* x, int dt, int64_t n, int* flag, hipStream_t st) {
  const int nb = (int)((n + kChunk - 1) / kChunk);
  if (nb <= 0) return;
  switch (dt) {
    case F32: hipLaunchKernelGGL((nonfinite_scan_kernel<float>), dim3(nb), dim3(kBlock), 0, st, (const float*)x, n, flag); break;
    case BF16: hipLaunchKernelGGL((nonfinite_scan_kernel<__bf16>), dim3(nb), dim3(kBlock), 0, st, (const __bf16*)x, n, flag); break;
    case F16: hipLaunchKernelGGL((nonfinite_scan_kernel<_Float16>), dim3(nb), dim3(kBlock), 0, st, (const _Float16*)x, n, flag); break;
  }
}

// -------------------------------------------------------------------------
// K6: fused optimizers on flat buckets.
// grad (TG: the wire / bucket dtype), fp32 master + fp32 state, and an optional
// low-precision model copy (TP) written in the same pass.  Arena segments are
// 64-element aligned, so the vector path covers everything but a final tail.
// SGD, Adam and Adadelta are a prologue and the arithmetic on one element, handed
// to flat_step (mv_flat_step.h: the loads, the stores, the alignment guard, the
// tail, and why LARS is not on it).
// -------------------------------------------------------------------------
namespace mv {

// The complements 1 - dampening, 1 - beta, 1 - rho (om*) are taken on the host in double and
// rounded once: 1.f - 0.999f is off by 1.3e-5 relative (the rounding of beta2, amplified by
// beta2 / (1 - beta2)), which put Adam's second moment 200 fp32 roundings away from torch's
// (tests/test_flat_kernels_gpu.py).
struct SgdHp { float lr, momentum, omd, wd, gscale; int nesterov, first; };
// Graph-replayable hyperparameters: when ``dyn`` is non-null the kernel reads the
// per-step values from device memory instead of its by-value launch arguments,
// so a captured HIP graph keeps following LR schedules and step counters:
// dyn = [lr, first (0/1), bias_correction1, bias_correction2] (fp32, 16 bytes),
// refreshed on the stream before every replay (mivod/torch/graphs.py).
struct AdamHp { float lr, b1, b2, omb1, omb2, eps, wd, gscale, bc1, bc2; int adamw, keras_eps; };
struct AdadeltaHp { float lr, rho, omr, eps, wd, gscale; };

template <typename TP>
__device__ __forceinline__ void store_model(TP* p, const float (&v)[8]) { store8(p, v); }

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void sgd_flat_kernel(const TG* __restrict__ g,
                                                           float* __restrict__ w,
                                                           float* __restrict__ mom,
                                                           TP* __restrict__ model, int64_t n,
                                                           SgdHp hp,
                                                           const float* __restrict__ dyn,
                                                           const int* __restrict__ skip,
                                                           const float* __restrict__ gclip) {
  if (skip && *skip) return;   // overflow guard: every rank skips this step identically
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.lr = dyn[0]; hp.first = dyn[1] != 0.f; }
  float* const st[1] = {mom};
  flat_step<1>(g, w, st, model, n, [&](float gj, float& wj, float& mj) {
    // g*gscale rounded, wd*w fused into the add: spelled out, because which product of
    // a*b + c*d -ffp-contract=fast fuses here follows the registers the two scales happen to
    // live in (with the gclip operand added the compiler fused the other one, and every
    // result of a step with weight decay moved by a rounding)
    float d = __builtin_fmaf(hp.wd, wj, gj * hp.gscale);
    if (mom) {
      float b = hp.first ? d : hp.momentum * mj + hp.omd * d;
      mj = b;
      d = hp.nesterov ? d + hp.momentum * b : b;
    }
    wj -= hp.lr * d;
  });
}

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void adam_flat_kernel(const TG* __restrict__ g,
                                                            float* __restrict__ w,
                                                            float* __restrict__ m,
                                                            float* __restrict__ v,
                                                            TP* __restrict__ model, int64_t n,
                                                            AdamHp hp,
                                                            const float* __restrict__ dyn,
                                                            const int* __restrict__ skip,
                                                            const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.lr = dyn[0]; hp.bc1 = dyn[2]; hp.bc2 = dyn[3]; }
  const float step = hp.lr / hp.bc1;
  const float rbc2 = 1.f / sqrtf(hp.bc2);
  // always given (the binding requires both): with flat_step's null tests left in, the
  // compiler fuses the m update through the other product in every second lane
  __builtin_assume(m && v);
  float* const st[2] = {m, v};
  flat_step<2>(g, w, st, model, n, [&](float gj, float& wj, float& mj, float& vj) {
    float gr = gj * hp.gscale;
    if (!hp.adamw) gr += hp.wd * wj;
    mj = hp.b1 * mj + hp.omb1 * gr;
    vj = hp.b2 * vj + hp.omb2 * gr * gr;
    if (hp.adamw) wj *= (1.f - hp.lr * hp.wd);
    // torch: m_hat / (sqrt(v_hat) + eps); Keras/TF: lr*sqrt(bc2)/bc1 * m / (sqrt(v) + eps)
    float denom = hp.keras_eps ? (sqrtf(vj) + hp.eps) * rbc2 : sqrtf(vj) * rbc2 + hp.eps;
    wj -= step * mj / denom;
  });
}

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void adadelta_flat_kernel(const TG* __restrict__ g,
                                                                float* __restrict__ w,
                                                                float* __restrict__ sq,
                                                                float* __restrict__ acc,
                                                                TP* __restrict__ model, int64_t n,
                                                                AdadeltaHp hp,
                                                                const float* __restrict__ dyn,
                                                                const int* __restrict__ skip,
                                                                const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) hp.lr = dyn[0];
  __builtin_assume(sq && acc);   // always given, as in adam_flat_kernel
  float* const st[2] = {sq, acc};
  flat_step<2>(g, w, st, model, n, [&](float gj, float& wj, float& sj, float& aj) {
    float gr = gj * hp.gscale + hp.wd * wj;
    sj = hp.rho * sj + hp.omr * gr * gr;
    float delta = sqrtf(aj + hp.eps) / sqrtf(sj + hp.eps) * gr;
    aj = hp.rho * aj + hp.omr * delta * delta;
    wj -= hp.lr * delta;
  });
}

// ---- segmented reductions (LARS norms, Adasum Gram terms) ----
// Chunk table (static per bucket layout): chunk c covers [begin[c], begin[c]+len[c])
// of segment seg[c]; chunks never straddle segments.  Pass 1 writes one partial
// per chunk (block-level, fixed-order => deterministic, so every rank computes
// bit-identical coefficients); pass 2 sums a segment's partials in chunk order.
template <typename TA, typename TB, int MODE>  // MODE 0: (a.a, b.b)  MODE 1: (a.b, a.a, b.b)
__global__ __launch_bounds__(kBlock) void seg_partial_kernel(const TA* __restrict__ a,
                                                              const TB* __restrict__ b,
                                                              const int64_t* __restrict__ cbeg,
                                                              const int32_t* __restrict__ clen,
                                                              float* __restrict__ partial,
                                                              float bscale,
                                                              const float* __restrict__ gclip) {
  constexpr int NV = MODE == 0 ? 2 : 3;
  bscale = clipped_gscale(bscale, gclip);   // LARS measures the norm of the clipped gradient
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  float s[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) s[k] = 0.f;
  const TA* ap = a + beg;
  const TB* bp = b + beg;
  const bool vec = aligned16(ap) && aligned16(bp) && (len % kVec) == 0;
  if (vec) {
    for (int i = threadIdx.x * kVec; i < len; i += kBlock * kVec) {
      float av[8], bv[8];
      load8(ap + i, av);
      load8(bp + i, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = av[j], y = bv[j] * bscale;
        if (MODE == 0) { s[0] += x * x; s[1] += y * y; }
        else { s[0] += x * y; s[1] += x * x; s[2] += y * y; }
      }
    }
  } else {
    for (int i = threadIdx.x; i < len; i += kBlock) {
      float x = ld1(ap + i), y = ld1(bp + i) * bscale;
      if (MODE == 0) { s[0] += x * x; s[1] += y * y; }
      else { s[0] += x * y; s[1] += x * x; s[2] += y * y; }
    }
  }
  block_sum<NV>(s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) partial[(int64_t)c * NV + k] = s[k];
  }
}

// swap (NV == 3 only): store (a.b, |b|^2, |a|^2) — the Adasum level kernels
// compute (f.r, |f|^2, |r|^2) where f may hold the UPPER group's vector b
template <int NV>
__global__ __launch_bounds__(kWave) void seg_reduce_kernel(const float* __restrict__ partial,
                                                            const int32_t* __restrict__ seg_c0,
                                                            const int32_t* __restrict__ seg_nc,
                                                            float* __restrict__ out, int swap) {
  const int s = blockIdx.x;
  const int c0 = seg_c0[s], nc = seg_nc[s];
  float v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.f;
  for (int c = threadIdx.x; c < nc; c += kWave) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += partial[(int64_t)(c0 + c) * NV + k];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] = wave_sum(v[k]);
    const int kk = (NV == 3 && swap && k > 0) ? 3 - k : k;
    if (threadIdx.x == 0) out[s * NV + kk] = v[k];
  }
}

struct LarsHp { float lr, momentum, wd, eta, gscale, eps; int first; };

// LARS: per-segment trust ratio eta*|w| / (|g| + wd*|w|); segments flagged
// (bit0) skip both adaptation and weight decay (BN / bias convention).
template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void lars_flat_kernel(const TG* __restrict__ g,
                                                            float* __restrict__ w,
                                                            float* __restrict__ mom,
                                                            TP* __restrict__ model,
                                                            const int64_t* __restrict__ cbeg,
                                                            const int32_t* __restrict__ clen,
                                                            const int32_t* __restrict__ cseg,
                                                            const int32_t* __restrict__ sflag,
                                                            const float* __restrict__ norms,
                                                            LarsHp hp,
                                                            const float* __restrict__ dyn,
                                                            const int* __restrict__ skip,
                                                            const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.lr = dyn[0]; hp.first = dyn[1] != 0.f; }
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  const int s = cseg[c];
  const bool skip_seg = sflag[s] & 1;
  const float wn = sqrtf(norms[2 * s]);
  const float gn = sqrtf(norms[2 * s + 1]);
  const float wd = skip_seg ? 0.f : hp.wd;
  float trust = 1.f;
  if (!skip_seg && wn > 0.f && gn > 0.f) trust = hp.eta * wn / (gn + wd * wn + hp.eps);
  const float slr = hp.lr * trust;
  // 8-wide vector body over the 16-byte-aligned prefix (arena segments are
  // 64-element aligned and chunks start on 4096-element boundaries), scalar tail
  const int nvec = (aligned16(g + beg) && aligned16(w + beg) && aligned16(mom + beg) &&
                    (!model || aligned16(model + beg))) ? (len / kVec) * kVec : 0;
  for (int i = threadIdx.x * kVec; i < nvec; i += kBlock * kVec) {
    const int64_t k = beg + i;
    float gv[8], wv[8], mv_[8];
    load8(g + k, gv);
    load8(w + k, wv);
    load8(mom + k, mv_);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = gv[j] * hp.gscale + wd * wv[j];
      float b = hp.first ? slr * d : hp.momentum * mv_[j] + slr * d;
      mv_[j] = b;
      wv[j] -= b;
    }
    store8(w + k, wv);
    store8(mom + k, mv_);
    if (model) store_model(model + k, wv);
  }
  for (int i = nvec + threadIdx.x; i < len; i += kBlock) {
    const int64_t k = beg + i;
    float wk = w[k];
    float d = ld1(g + k) * hp.gscale + wd * wk;
    float b = hp.first ? slr * d : hp.momentum * mom[k] + slr * d;
    mom[k] = b;
    wk -= b;
    w[k] = wk;
    if (model) st1(model + k, wk);
  }
}

// LAMB (You et al. 2019): Adam moments, then per segment w -= lr * (|w| / |u|) * u with
// u = m_hat / (sqrt(v_hat) + eps) + wd * w.  Two streaming kernels over the chunk table with
// seg_reduce_kernel<2> between them; segments flagged (bit0) take wd = 0 and trust 1, as in
// lars_flat_kernel.  Bias correction is always on.
struct LambHp { float lr, b1, b2, omb1, omb2, eps, wd, gscale, bc1, bc2; };

// The update direction of one element from the UPDATED moments and the master BEFORE its
// update; rbc1 = 1 / bc1, rbc2 = 1 / sqrt(bc2).  Stage 1 measures |u| and stage 2 applies u
// recomputed from the stored m and v, so both go through this one expression; the two
// fused multiply-adds are spelled out so that neither call site can be contracted
// differently from the other: the norm that was measured is the norm of what is applied.
__device__ __forceinline__ float lamb_u(float m, float v, float w, float rbc1, float rbc2,
                                        float eps, float wd) {
  const float den = __builtin_fmaf(sqrtf(v), rbc2, eps);
  return __builtin_fmaf(wd, w, m * rbc1 / den);
}

// Stage 1: m and v in place, one (sum w^2, sum u^2) partial per chunk in fixed order.
template <typename TG>
__global__ __launch_bounds__(kBlock) void lamb_moments_kernel(const TG* __restrict__ g,
                                                               const float* __restrict__ w,
                                                               float* __restrict__ m,
                                                               float* __restrict__ v,
                                                               const int64_t* __restrict__ cbeg,
                                                               const int32_t* __restrict__ clen,
                                                               const int32_t* __restrict__ cseg,
                                                               const int32_t* __restrict__ sflag,
                                                               float* __restrict__ partial,
                                                               LambHp hp,
                                                               const float* __restrict__ dyn,
                                                               const int* __restrict__ skip,
                                                               const float* __restrict__ gclip) {
  if (skip && *skip) return;   // uniform: no lane reaches block_sum's barrier
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.bc1 = dyn[2]; hp.bc2 = dyn[3]; }
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  const float wd = (sflag[cseg[c]] & 1) ? 0.f : hp.wd;
  const float rbc1 = 1.f / hp.bc1;
  const float rbc2 = 1.f / sqrtf(hp.bc2);
  float acc[2] = {0.f, 0.f};
  // the same body layout as lars_flat_kernel: vector prefix where every operand is
  // 16-byte aligned, scalar tail (all of the chunk at an unaligned offset)
  const int nvec = (aligned16(g + beg) && aligned16(w + beg) && aligned16(m + beg) &&
                    aligned16(v + beg)) ? (len / kVec) * kVec : 0;
  for (int i = threadIdx.x * kVec; i < nvec; i += kBlock * kVec) {
    const int64_t k = beg + i;
    float gv[8], wv[8], mv_[8], vv[8];
    load8(g + k, gv);
    load8(w + k, wv);
    load8(m + k, mv_);
    load8(v + k, vv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gr = gv[j] * hp.gscale;
      mv_[j] = hp.b1 * mv_[j] + hp.omb1 * gr;
      vv[j] = hp.b2 * vv[j] + hp.omb2 * gr * gr;
      const float u = lamb_u(mv_[j], vv[j], wv[j], rbc1, rbc2, hp.eps, wd);
      acc[0] += wv[j] * wv[j];
      acc[1] += u * u;
    }
    store8(m + k, mv_);
    store8(v + k, vv);
  }
  for (int i = nvec + threadIdx.x; i < len; i += kBlock) {
    const int64_t k = beg + i;
    const float wk = w[k];
    const float gr = ld1(g + k) * hp.gscale;
    const float mk = hp.b1 * m[k] + hp.omb1 * gr;
    const float vk = hp.b2 * v[k] + hp.omb2 * gr * gr;
    m[k] = mk;
    v[k] = vk;
    const float u = lamb_u(mk, vk, wk, rbc1, rbc2, hp.eps, wd);
    acc[0] += wk * wk;
    acc[1] += u * u;
  }
  block_sum<2>(acc);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)c] = acc[0];
    partial[2 * (int64_t)c + 1] = acc[1];
  }
}

// Stage 2: trust from the segment's norms, w -= lr * trust * u, the model copy.
template <typename TP>
__global__ __launch_bounds__(kBlock) void lamb_apply_kernel(float* __restrict__ w,
                                                             const float* __restrict__ m,
                                                             const float* __restrict__ v,
                                                             TP* __restrict__ model,
                                                             const int64_t* __restrict__ cbeg,
                                                             const int32_t* __restrict__ clen,
                                                             const int32_t* __restrict__ cseg,
                                                             const int32_t* __restrict__ sflag,
                                                             const float* __restrict__ norms,
                                                             LambHp hp,
                                                             const float* __restrict__ dyn,
                                                             const int* __restrict__ skip) {
  if (skip && *skip) return;
  if (dyn) { hp.lr = dyn[0]; hp.bc1 = dyn[2]; hp.bc2 = dyn[3]; }
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  const int s = cseg[c];
  const bool plain = sflag[s] & 1;
  const float wd = plain ? 0.f : hp.wd;
  const float wn = sqrtf(norms[2 * s]);
  const float un = sqrtf(norms[2 * s + 1]);
  float trust = 1.f;
  if (!plain && wn > 0.f && un > 0.f) trust = wn / un;
  const float slr = hp.lr * trust;
  const float rbc1 = 1.f / hp.bc1;
  const float rbc2 = 1.f / sqrtf(hp.bc2);
  const int nvec = (aligned16(w + beg) && aligned16(m + beg) && aligned16(v + beg) &&
                    (!model || aligned16(model + beg))) ? (len / kVec) * kVec : 0;
  for (int i = threadIdx.x * kVec; i < nvec; i += kBlock * kVec) {
    const int64_t k = beg + i;
    float wv[8], mv_[8], vv[8];
    load8(w + k, wv);
    load8(m + k, mv_);
    load8(v + k, vv);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      wv[j] -= slr * lamb_u(mv_[j], vv[j], wv[j], rbc1, rbc2, hp.eps, wd);
    store8(w + k, wv);
    if (model) store_model(model + k, wv);
  }
  for (int i = nvec + threadIdx.x; i < len; i += kBlock) {
    const int64_t k = beg + i;
    float wk = w[k];
    wk -= slr * lamb_u(m[k], v[k], wk, rbc1, rbc2, hp.eps, wd);
    w[k] = wk;
    if (model) st1(model + k, wk);
  }
}

// Adasum merge: a <- ca*a + cb*b with ca = 1 - a.b/(2|a|^2), cb = 1 - a.b/(2|b|^2)
template <typename T>
__global__ __launch_bounds__(kBlock) void adasum_combine_kernel(T* __restrict__ a,
                                                                 const T* __restrict__ b,
                                                                 const int64_t* __restrict__ cbeg,
                                                                 const int32_t* __restrict__ clen,
                                                                 const int32_t* __restrict__ cseg,
                                                                 const float* __restrict__ dots) {
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  const int s = cseg[c];
  const float dot = dots[3 * s], na = dots[3 * s + 1], nb = dots[3 * s + 2];
  const float ca = na >= 1e-8f ? 1.f - dot / (2.f * na) : 1.f;
  const float cb = nb >= 1e-8f ? 1.f - dot / (2.f * nb) : 1.f;
  T* ap = a + beg;
  const T* bp = b + beg;
  if (aligned16(ap) && aligned16(bp) && (len % kVec) == 0) {
    for (int i = threadIdx.x * kVec; i < len; i += kBlock * kVec) {
      float av[8], bv[8];
      load8(ap + i, av);
      load8(bp + i, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = ca * av[j] + cb * bv[j];
      store8(ap + i, av);
    }
  } else {
    for (int i = threadIdx.x; i < len; i += kBlock) st1(ap + i, ca * ld1(ap + i) + cb * ld1(bp + i));
  }
}

// Vector-halving Adasum merge of one level (mivod/parallel/adasum.py):
//   f <- cf * fin + cr * r   over the chunks of the level's kept range
// fin is the fp32 running merge (== f, in place) or, at level 0, the wire-dtype
// bucket itself (f = fp32(bucket) exactly, so no separate cast pass); r is the
// partner's wire copy.  The per-segment Gram terms (a.b, |a|^2, |b|^2) arrive as
// `nrows` partial rows (one per rank of the level's group, row stride
// `row_stride` floats) and are summed here in FIXED row order, so every rank of
// the group derives bit-identical coefficients.  swap == 0: f holds the lower
// group's vector a (cf = ca); swap == 1: f holds b.
// emit (nullable, wire dtype): elements with absolute index in [elo, ehi) are
// also written as cast(f) — the next level's outgoing half (or, at the last
// level, the finished piece straight into the bucket), fusing the wire cast.
// fin may alias f or emit (each element is read, then written, by one thread).
template <typename TF, typename TB>
__global__ __launch_bounds__(kBlock) void adasum_merge_kernel(const TF* fin, float* f,
                                                               const TB* __restrict__ r,
                                                               const int64_t* __restrict__ cbeg,
                                                               const int32_t* __restrict__ clen,
                                                               const int32_t* __restrict__ cseg,
                                                               const float* __restrict__ rows,
                                                               int nrows, int row_stride, int swap,
                                                               TB* emit, int64_t elo, int64_t ehi) {
  const int c = blockIdx.x;
  const int64_t beg = cbeg[c];
  const int len = clen[c];
  const int s = cseg[c];
  float dot = 0.f, na = 0.f, nb = 0.f;
  for (int g = 0; g < nrows; ++g) {
    const float* q = rows + (int64_t)g * row_stride + 3 * s;
    dot += q[0];
    na += q[1];
    nb += q[2];
  }
  const float ca = na >= 1e-8f ? 1.f - dot / (2.f * na) : 1.f;
  const float cb = nb >= 1e-8f ? 1.f - dot / (2.f * nb) : 1.f;
  const float cf = swap ? cb : ca;
  const float cr = swap ? ca : cb;
  const TF* ip = fin + beg;
  float* fp = f + beg;
  const TB* rp = r + beg;
  const bool em_any = emit != nullptr && beg < ehi && beg + len > elo;
  if (aligned16(ip) && aligned16(fp) && aligned16(rp) && (len % kVec) == 0) {
    for (int i = threadIdx.x * kVec; i < len; i += kBlock * kVec) {
      float fv[8], rv[8];
      load8(ip + i, fv);
      load8(rp + i, rv);
#pragma unroll
      for (int j = 0; j < 8; ++j) fv[j] = cf * fv[j] + cr * rv[j];
      store8(fp + i, fv);
      if (em_any) {
        const int64_t k = beg + i;
        if (k >= elo && k + kVec <= ehi && aligned16(emit + k)) {
          store8(emit + k, fv);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k + j >= elo && k + j < ehi) st1(emit + k + j, fv[j]);
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < len; i += kBlock) {
      const float v = cf * ld1(ip + i) + cr * ld1(rp + i);
      fp[i] = v;
      if (em_any && beg + i >= elo && beg + i < ehi) st1(emit + beg + i, v);
    }
  }
}

}  // namespace mv

// ---------------- host launchers (MV_GRID, DISPATCH_GP: mv_flat_step.h) ----------------
void mv_launch_sgd(const void* g, int gd, float* w, float* mom, void* model, int md, int64_t n,
                   float lr, float momentum, double dampening, float wd, float gscale, int nesterov,
                   int first, const float* dyn, const int* skip, const float* gclip,
                   hipStream_t st) {
  if (n <= 0) return;
  SgdHp hp{lr, momentum, (float)(1.0 - dampening), wd, gscale, nesterov, first};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((sgd_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, mom, (TP*)model, n, hp, dyn, skip,
                                         gclip));
}

void mv_launch_adam(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                    int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                    float bc1, float bc2, int adamw, int keras_eps, const float* dyn,
                    const int* skip, const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  AdamHp hp{lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, wd, gscale,
            bc1, bc2, adamw, keras_eps};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((adam_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, m, v, (TP*)model, n, hp, dyn, skip,
                                         gclip));
}

void mv_launch_adadelta(const void* g, int gd, float* w, float* sq, float* acc, void* model,
                        int md, int64_t n, float lr, double rho, float eps, float wd, float gscale,
                        const float* dyn, const int* skip, const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  AdadeltaHp hp{lr, (float)rho, (float)(1.0 - rho), eps, wd, gscale};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((adadelta_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock),
                                         0, st, (const TG*)g, w, sq, acc, (TP*)model, n, hp, dyn,
                                         skip, gclip));
}

void mv_launch_lars(const void* g, int gd, float* w, float* mom, void* model, int md,
                    const ChunkTable& ct, const int32_t* sflag, float* partial, float* norms,
                    float lr, float momentum, float wd, float eta, float gscale, float eps,
                    int first, const float* dyn, const int* skip, const float* gclip,
                    hipStream_t st) {
  if (ct.nchunks <= 0) return;
  // pass 1: per-chunk (|w|^2, |g|^2)
  switch (gd) {
    case F32: hipLaunchKernelGGL((seg_partial_kernel<float, float, 0>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const float*)w, (const float*)g, ct.begin, ct.len, partial, gscale, gclip); break;
    case BF16: hipLaunchKernelGGL((seg_partial_kernel<float, __bf16, 0>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const float*)w, (const __bf16*)g, ct.begin, ct.len, partial, gscale, gclip); break;
    case F16: hipLaunchKernelGGL((seg_partial_kernel<float, _Float16, 0>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const float*)w, (const _Float16*)g, ct.begin, ct.len, partial, gscale, gclip); break;
  }
  hipLaunchKernelGGL((seg_reduce_kernel<2>), dim3(ct.nseg), dim3(kWave), 0, st, partial, ct.seg_c0,
                     ct.seg_nc, norms, 0);
  // norms[2s+1] already includes gscale (bscale in pass 1) and the clip coefficient
  LarsHp hp{lr, momentum, wd, eta, gscale, eps, first};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((lars_flat_kernel<TG, TP>), dim3(ct.nchunks), dim3(kBlock),
                                         0, st, (const TG*)g, w, mom, (TP*)model, ct.begin, ct.len,
                                         ct.seg, sflag, norms, hp, dyn, skip, gclip));
}

void mv_launch_lamb(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                    const ChunkTable& ct, const int32_t* sflag, float* partial, float* norms,
                    float lr, double b1, double b2, float eps, float wd, float gscale, float bc1,
                    float bc2, const float* dyn, const int* skip, const float* gclip,
                    hipStream_t st) {
  if (ct.nchunks <= 0) return;
  LambHp hp{lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, wd, gscale,
            bc1, bc2};
  // stage 1: m, v and per-chunk (|w|^2, |u|^2)
#define MV_LAMB1(TG)                                                                            \
  hipLaunchKernelGGL((lamb_moments_kernel<TG>), dim3(ct.nchunks), dim3(kBlock), 0, st,           \
                     (const TG*)g, (const float*)w, m, v, ct.begin, ct.len, ct.seg, sflag,       \
                     partial, hp, dyn, skip, gclip)
  switch (gd) {
    case F32: MV_LAMB1(float); break;
    case BF16: MV_LAMB1(__bf16); break;
    case F16: MV_LAMB1(_Float16); break;
  }
#undef MV_LAMB1
  hipLaunchKernelGGL((seg_reduce_kernel<2>), dim3(ct.nseg), dim3(kWave), 0, st, partial, ct.seg_c0,
                     ct.seg_nc, norms, 0);
  // stage 2: the update, from the stored m and v (the gradient is not read again)
#define MV_LAMB2(TP)                                                                            \
  hipLaunchKernelGGL((lamb_apply_kernel<TP>), dim3(ct.nchunks), dim3(kBlock), 0, st, w,          \
                     (const float*)m, (const float*)v, (TP*)model, ct.begin, ct.len, ct.seg,     \
                     sflag, (const float*)norms, hp, dyn, skip)
  switch (md) {
    case F32: MV_LAMB2(float); break;
    case BF16: MV_LAMB2(__bf16); break;
    case F16: MV_LAMB2(_Float16); break;
  }
#undef MV_LAMB2
}

void mv_launch_seg_dot3(const void* a, const void* b, int dt, const ChunkTable& ct, float* partial,
                        float* out, int swap, hipStream_t st) {
  if (ct.nchunks <= 0) return;
  switch (dt) {
    case F32: hipLaunchKernelGGL((seg_partial_kernel<float, float, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const float*)a, (const float*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
    case BF16: hipLaunchKernelGGL((seg_partial_kernel<__bf16, __bf16, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const __bf16*)a, (const __bf16*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
    case F16: hipLaunchKernelGGL((seg_partial_kernel<_Float16, _Float16, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, (const _Float16*)a, (const _Float16*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
  }
  hipLaunchKernelGGL((seg_reduce_kernel<3>), dim3(ct.nseg), dim3(kWave), 0, st, partial, ct.seg_c0,
                     ct.seg_nc, out, swap);
}

void mv_launch_seg_dot3_f(const float* a, const void* b, int bdt, const ChunkTable& ct,
                          float* partial, float* out, int swap, hipStream_t st) {
  if (ct.nchunks <= 0) return;
  switch (bdt) {
    case F32: hipLaunchKernelGGL((seg_partial_kernel<float, float, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, a, (const float*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
    case BF16: hipLaunchKernelGGL((seg_partial_kernel<float, __bf16, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, a, (const __bf16*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
    case F16: hipLaunchKernelGGL((seg_partial_kernel<float, _Float16, 1>), dim3(ct.nchunks), dim3(kBlock), 0, st, a, (const _Float16*)b, ct.begin, ct.len, partial, 1.f, nullptr); break;
  }
  hipLaunchKernelGGL((seg_reduce_kernel<3>), dim3(ct.nseg), dim3(kWave), 0, st, partial, ct.seg_c0,
                     ct.seg_nc, out, swap);
}

void mv_launch_adasum_merge(const void* fin, int fdt, float* f, const void* r, int rdt,
                            const ChunkTable& ct, const float* rows, int nrows, int row_stride,
                            int swap, void* emit, int64_t elo, int64_t ehi, hipStream_t st) {
  if (ct.nchunks <= 0) return;
#define MV_MERGE(TF, TB)                                                                      \
  hipLaunchKernelGGL((adasum_merge_kernel<TF, TB>), dim3(ct.nchunks), dim3(kBlock), 0, st,     \
                     (const TF*)fin, f, (const TB*)r, ct.begin, ct.len, ct.seg, rows, nrows,   \
                     row_stride, swap, (TB*)emit, elo, ehi)
  if (fdt == F32) {
    switch (rdt) {
      case F32: MV_MERGE(float, float); break;
      case BF16: MV_MERGE(float, __bf16); break;
      case F16: MV_MERGE(float, _Float16); break;
    }
  } else if (fdt == BF16 && rdt == BF16) {
    MV_MERGE(__bf16, __bf16);
  } else if (fdt == F16 && rdt == F16) {
    MV_MERGE(_Float16, _Float16);
  }
#undef MV_MERGE
}

void mv_launch_adasum_fcombine(float* f, const void* r, int rdt, const ChunkTable& ct,
                               const float* dots, int swap, hipStream_t st) {
  mv_launch_adasum_merge(f, F32, f, r, rdt, ct, dots, 1, 0, swap, nullptr, 0, 0, st);
}

void mv_launch_adasum_combine(void* a, const void* b, int dt, const ChunkTable& ct,
                              const float* dots, hipStream_t st) {
  if (ct.nchunks <= 0) return;
  switch (dt) {
    case F32: hipLaunchKernelGGL((adasum_combine_kernel<float>), dim3(ct.nchunks), dim3(kBlock), 0, st, (float*)a, (const float*)b, ct.begin, ct.len, ct.seg, dots); break;
    case BF16: hipLaunchKernelGGL((adasum_combine_kernel<__bf16>), dim3(ct.nchunks), dim3(kBlock), 0, st, (__bf16*)a, (const __bf16*)b, ct.begin, ct.len, ct.seg, dots); break;
    case F16: hipLaunchKernelGGL((adasum_combine_kernel<_Float16>), dim3(ct.nchunks), dim3(kBlock), 0, st, (_Float16*)a, (const _Float16*)b, ct.begin, ct.len, ct.seg, dots); break;
  }
}
