// Host-side declarations of the RMSprop / Adagrad flat-bucket launchers (mv_adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Both steps take the operands of the other flat optimizers (mv_kernels.h): the gradient in the
// wire dtype gd, the fp32 master w and fp32 state, an optional model copy in dtype md written in
// the same pass, dyn (nullable; dyn[0] replaces lr), skip (nullable; nonzero => nothing is
// written) and gclip (nullable; gscale is multiplied by gclip[0]).  A base pointer that is not 16-byte aligned sends the whole launch down the scalar
// path.

// torch.optim.RMSprop: sq = alpha*sq + (1-alpha)*gr^2 with gr = g*gscale + wd*w;
// ga (nullable: centered) = alpha*ga + (1-alpha)*gr and avg = sqrt(max(sq - ga^2, 0)) + eps,
// else avg = sqrt(sq) + eps; buf (nullable: momentum) = momentum*buf + gr/avg and w -= lr*buf,
// else w -= lr*gr/avg.  alpha arrives as a double: 1 - alpha is rounded to fp32 once.
void mv_launch_rmsprop(const void* g, int gd, float* w, float* sq, float* ga, float* buf,
                       void* model, int md, int64_t n, float lr, double alpha, float eps, float wd,
                       float momentum, float gscale, const float* dyn, const int* skip,
                       const float* gclip, hipStream_t st);
// torch.optim.Adagrad: sum += gr^2, w -= lr * gr / (sqrt(sum) + eps); lr is the decayed rate
// lr0 / (1 + (step-1)*lr_decay), taken by the caller in double.  sum must not be null: the
// kernel tells the compiler so (__builtin_assume).
void mv_launch_adagrad(const void* g, int gd, float* w, float* sum, void* model, int md, int64_t n,
                       float lr, float eps, float wd, float gscale, const float* dyn,
                       const int* skip, const float* gclip, hipStream_t st);
