// Host-side declarations of the Adam-family flat-bucket launchers of mv_adamfam.hip: Adam /
// AdamW with amsgrad, Adamax and NAdam.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// All three take the operands of the other flat optimizers (mv_kernels.h): the gradient in the
// wire dtype gd, the fp32 master w and fp32 state, an optional model copy in dtype md written in
// the same pass, dyn (nullable; the device hyperparameter block of a HIP-graph replay), skip
// (nullable; nonzero => nothing is written) and gclip (nullable; gscale is multiplied by
// gclip[0]).  A base pointer that is not 16-byte aligned sends the whole launch down the scalar
// path.  The state pointers must not be null: the kernels tell the compiler so
// (__builtin_assume).  The betas arrive as doubles: 1 - beta is rounded to fp32 once.

// mv_launch_adam's rule with vmax = max(vmax, v) (on the uncorrected v, as torch and Keras do)
// in place of v in the denominator, for both epsilon placements.  dyn = [lr, -, bc1, bc2].
void mv_launch_adam_amsgrad(const void* g, int gd, float* w, float* m, float* v, float* vmax,
                            void* model, int md, int64_t n, float lr, double b1, double b2,
                            float eps, float wd, float gscale, float bc1, float bc2, bool adamw,
                            bool keras_eps, const float* dyn, const int* skip, const float* gclip,
                            hipStream_t st);
// torch.optim.Adamax: gr = g*gscale + wd*w, m = b1*m + (1-b1)*gr, u = max(b2*u, |gr| + eps),
// w -= lr/bc1 * m/u; keras_eps: u = max(b2*u, |gr|), w -= lr/bc1 * m/(u + eps).  An element
// whose divisor is exactly 0 takes no update.  dyn = [lr, -, bc1, -].
void mv_launch_adamax(const void* g, int gd, float* w, float* m, float* u, void* model, int md,
                      int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                      float bc1, bool keras_eps, const float* dyn, const int* skip,
                      const float* gclip, hipStream_t st);
// torch.optim.NAdam: m and v as in Adam, denom = sqrt(v/bc2) + eps,
// w -= lr*cg*gr/denom + lr*cm*m/denom with cg = (1-mu_t)/(1-P_t) and
// cm = mu_{t+1}/(1 - P_t*mu_{t+1}), both taken by the caller in double.  adamw: the decoupled
// decay w *= 1 - lr*wd.  dyn = [lr, cg, cm, bc2].
void mv_launch_nadam(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                     int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                     float cg, float cm, float bc2, bool adamw, const float* dyn, const int* skip,
                     const float* gclip, hipStream_t st);
