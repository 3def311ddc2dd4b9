// Host-side declarations of the weight-averaging launchers (mv_ema.hip): the fp32 exponential
// moving average of the fp32 master weights (ema_decay of the mivod.optim.Fused* optimizers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// All three run over the flat range [0, n) of w (fp32 master), e (fp32 average) and, where
// model is not null, the low-precision model copy of model_dtype (mv::Dtype).  skip is the
// nullable device flag of the K6 step kernels: nonzero, the launch stores nothing.
//
// update:    e[i] = e[i] + omd * (w[i] - e[i]); omd == 1.0f stores w[i] itself.  w is only read.
void mv_launch_ema_update(const float* w, float* e, int64_t n, float omd, const int* skip,
                          hipStream_t st);
// swap:      (w[i], e[i]) = (e[i], w[i]); model[i] = cast(new w[i])
void mv_launch_ema_swap(float* w, float* e, void* model, int model_dtype, int64_t n,
                        const int* skip, hipStream_t st);
// overwrite: w[i] = e[i]; model[i] = cast(e[i]).  e is only read.
void mv_launch_ema_overwrite(float* w, const float* e, void* model, int model_dtype, int64_t n,
                             const int* skip, hipStream_t st);
