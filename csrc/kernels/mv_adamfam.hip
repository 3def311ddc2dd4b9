// mivod gfx950 kernels: the rest of the Adam family on flat buckets (K6, next to
// mv_kernels.hip's Adam and mv_adaptive.hip's RMSprop / Adagrad): Adam / AdamW with amsgrad,
// Adamax and NAdam.  Pure streaming updates on mv_flat_step.h's skeleton: one workgroup of 256
// lanes per 4096-element chunk, 8 elements per lane per step, the gradient read once in the
// wire dtype (TG), fp32 master and state read and written once, the optional low-precision
// model copy (TP) written in the same pass.  Each kernel is a prologue and the arithmetic on
// one element, which therefore exists exactly once: a result does not depend on n % 8 or on
// the alignment of the operands (an offset view goes down the skeleton's scalar path).
//
// Bytes per element with an fp16 wire and a bf16 model: g 2 + w 4+4 + model 2 = 12, plus 8 per
// state buffer: 28 (Adamax, NAdam: as Adam), 36 (amsgrad).
//
// Every a*b + c*d below is written as one __builtin_fmaf around the rounded other product:
// which of the two -ffp-contract=fast fuses otherwise follows the register allocation
// (mv_flat_step.h, sgd_flat_kernel), and these kernels have no earlier bits to keep.
//
// Resources of every instantiation (hipcc --offload-arch=gfx950 -O3,
// -Rpass-analysis=kernel-resource-usage; TG = gradient, TP = model; scratch is 0 bytes and
// LDS 0 bytes in all 27).  Occupancy is waves per SIMD.
//
//   TG / TP        amsgrad (NS 3)     adamax (NS 2)      nadam (NS 2)
//                  VGPRs  occ.        VGPRs  occ.        VGPRs  occ.
//   fp32 / fp32     62     8           52     8           54     8
//   bf16 / fp32     64     8           52     8           54     8
//   fp16 / fp32     64     8           52     8           54     8
//   fp32 / bf16     72     7           58     8           60     8
//   bf16 / bf16     74     6           58     8           60     8
//   fp16 / bf16     74     6           58     8           60     8
//   fp32 / fp16     72     7           58     8           60     8
//   bf16 / fp16     74     6           58     8           60     8
//   fp16 / fp16     74     6           58     8           60     8
//
// (a launch without a model copy is the fp32-model instantiation.)  Adamax and NAdam sit where
// adam_flat_kernel sits (54 / 60 VGPRs, 8 waves).  amsgrad's third stream costs 8 data
// registers and an address pair and crosses an occupancy step with a 16-bit model copy:
// 8 -> 7 or 6 waves per SIMD.  The same loop written out by hand, as rmsprop_flat_kernel is,
// compiles to 64 / 74 VGPRs (8 / 6 waves): no lower in any instantiation, so there is nothing
// for it to win and the skeleton stays.  6 waves per SIMD is where the 36-byte RMSprop
// (momentum and centered, 79 VGPRs) streams within 2% of its byte prediction.
#include "mv_adamfam.h"
#include "mv_flat_step.h"

using namespace mv;

namespace mv {

// om* = 1 - beta, taken on the host in double and rounded once (mv_kernels.hip, at SgdHp)
struct AmsgradHp { float lr, b1, b2, omb1, omb2, eps, wd, gscale, bc1, bc2; int adamw, keras_eps; };
struct AdamaxHp { float lr, b1, b2, omb1, eps, wd, gscale, bc1; int keras_eps; };
struct NadamHp { float lr, b1, b2, omb1, omb2, eps, wd, gscale, cg, cm, bc2; int adamw; };

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void adam_amsgrad_flat_kernel(
    const TG* __restrict__ g, float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ vmax, TP* __restrict__ model, int64_t n, AmsgradHp hp,
    const float* __restrict__ dyn, const int* __restrict__ skip, const float* __restrict__ gclip) {
  if (skip && *skip) return;   // overflow guard: every rank skips this step identically
  hp.gscale = clipped_gscale(hp.gscale, gclip);   // global-norm clip coefficient (mv_clip.hip)
  if (dyn) { hp.lr = dyn[0]; hp.bc1 = dyn[2]; hp.bc2 = dyn[3]; }
  const float step = hp.lr / hp.bc1;
  const float rbc2 = 1.f / sqrtf(hp.bc2);
  const float decay = 1.f - hp.lr * hp.wd;
  __builtin_assume(m && v && vmax);   // always given: drops flat_step's null tests, as in Adam
  float* const st[3] = {m, v, vmax};
  flat_step<3>(g, w, st, model, n, [&](float gj, float& wj, float& mj, float& vj, float& xj) {
    float gr = gj * hp.gscale;
    if (!hp.adamw) gr = __builtin_fmaf(hp.wd, wj, gr);
    mj = __builtin_fmaf(hp.b1, mj, hp.omb1 * gr);
    vj = __builtin_fmaf(hp.b2, vj, hp.omb2 * gr * gr);
    xj = fmaxf(xj, vj);   // on the uncorrected v, as torch and Keras take it
    if (hp.adamw) wj *= decay;
    // torch: m_hat / (sqrt(vmax_hat) + eps); Keras/TF: the eps inside the bias correction
    const float root = sqrtf(xj);
    const float denom = hp.keras_eps ? (root + hp.eps) * rbc2 : root * rbc2 + hp.eps;
    wj -= step * mj / denom;
  });
}

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void adamax_flat_kernel(const TG* __restrict__ g,
                                                              float* __restrict__ w,
                                                              float* __restrict__ m,
                                                              float* __restrict__ u,
                                                              TP* __restrict__ model, int64_t n,
                                                              AdamaxHp hp,
                                                              const float* __restrict__ dyn,
                                                              const int* __restrict__ skip,
                                                              const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.lr = dyn[0]; hp.bc1 = dyn[2]; }
  const float step = hp.lr / hp.bc1;
  // torch's placement: eps joins |gr| inside the max; Keras': it joins u in the divisor
  const float eps_in = hp.keras_eps ? 0.f : hp.eps;
  const float eps_out = hp.keras_eps ? hp.eps : 0.f;
  __builtin_assume(m && u);
  float* const st[2] = {m, u};
  flat_step<2>(g, w, st, model, n, [&](float gj, float& wj, float& mj, float& uj) {
    const float gr = __builtin_fmaf(hp.wd, wj, gj * hp.gscale);
    mj = __builtin_fmaf(hp.b1, mj, hp.omb1 * gr);
    uj = fmaxf(hp.b2 * uj, fabsf(gr) + eps_in);   // adding 0.f is exact
    const float d = uj + eps_out;
    // a divisor of exactly 0 (eps = 0 and an all-zero history): the element takes no update,
    // where torch's 0/0 is NaN
    if (d != 0.f) wj -= step * mj / d;
  });
}

template <typename TG, typename TP>
__global__ __launch_bounds__(kBlock) void nadam_flat_kernel(const TG* __restrict__ g,
                                                             float* __restrict__ w,
                                                             float* __restrict__ m,
                                                             float* __restrict__ v,
                                                             TP* __restrict__ model, int64_t n,
                                                             NadamHp hp,
                                                             const float* __restrict__ dyn,
                                                             const int* __restrict__ skip,
                                                             const float* __restrict__ gclip) {
  if (skip && *skip) return;
  hp.gscale = clipped_gscale(hp.gscale, gclip);
  if (dyn) { hp.lr = dyn[0]; hp.cg = dyn[1]; hp.cm = dyn[2]; hp.bc2 = dyn[3]; }
  const float sg = hp.lr * hp.cg;   // the weight of the gradient and of the momentum in the
  const float sm = hp.lr * hp.cm;   // Nesterov step
  const float rbc2 = 1.f / sqrtf(hp.bc2);
  const float decay = 1.f - hp.lr * hp.wd;
  __builtin_assume(m && v);
  float* const st[2] = {m, v};
  flat_step<2>(g, w, st, model, n, [&](float gj, float& wj, float& mj, float& vj) {
    float gr = gj * hp.gscale;
    if (!hp.adamw) gr = __builtin_fmaf(hp.wd, wj, gr);
    mj = __builtin_fmaf(hp.b1, mj, hp.omb1 * gr);
    vj = __builtin_fmaf(hp.b2, vj, hp.omb2 * gr * gr);
    if (hp.adamw) wj *= decay;
    const float denom = sqrtf(vj) * rbc2 + hp.eps;   // sqrt(v / bc2) + eps
    // lr*cg*gr/denom + lr*cm*m/denom over the one quotient
    wj -= __builtin_fmaf(sg, gr, sm * mj) / denom;
  });
}

}  // namespace mv

// ---------------- host launchers (MV_GRID, DISPATCH_GP: mv_flat_step.h) ----------------
void mv_launch_adam_amsgrad(const void* g, int gd, float* w, float* m, float* v, float* vmax,
                            void* model, int md, int64_t n, float lr, double b1, double b2,
                            float eps, float wd, float gscale, float bc1, float bc2, bool adamw,
                            bool keras_eps, const float* dyn, const int* skip, const float* gclip,
                            hipStream_t st) {
  if (n <= 0) return;
  AmsgradHp hp{lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, wd, gscale,
               bc1, bc2, adamw ? 1 : 0, keras_eps ? 1 : 0};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((adam_amsgrad_flat_kernel<TG, TP>), MV_GRID(n),
                                         dim3(kBlock), 0, st, (const TG*)g, w, m, v, vmax,
                                         (TP*)model, n, hp, dyn, skip, gclip));
}

void mv_launch_adamax(const void* g, int gd, float* w, float* m, float* u, void* model, int md,
                      int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                      float bc1, bool keras_eps, const float* dyn, const int* skip,
                      const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  AdamaxHp hp{lr, (float)b1, (float)b2, (float)(1.0 - b1), eps, wd, gscale, bc1,
              keras_eps ? 1 : 0};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((adamax_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, m, u, (TP*)model, n, hp, dyn, skip,
                                         gclip));
}

void mv_launch_nadam(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                     int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                     float cg, float cm, float bc2, bool adamw, const float* dyn, const int* skip,
                     const float* gclip, hipStream_t st) {
  if (n <= 0) return;
  NadamHp hp{lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, wd, gscale, cg,
             cm, bc2, adamw ? 1 : 0};
  DISPATCH_GP(gd, md, hipLaunchKernelGGL((nadam_flat_kernel<TG, TP>), MV_GRID(n), dim3(kBlock), 0,
                                         st, (const TG*)g, w, m, v, (TP*)model, n, hp, dyn, skip,
                                         gclip));
}
