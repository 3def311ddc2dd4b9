// Host-side declarations of the global gradient-norm clipping launchers (mv_clip.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// partial[b] = sum of x[b*4096 : (b+1)*4096)^2 in fp32 for every 4096-element chunk b of
// x[0:n) (written, not accumulated: ceil(n / 4096) entries), each chunk reduced in a fixed
// order, so equal inputs give equal bits on every rank and in every launch.  flag (nullable):
// |= any(!isfinite(x)), as mv_launch_nonfinite_scan.  Read-only on x.
void mv_launch_grad_sumsq(const void* x, int dtype, int64_t n, float* partial, int* flag,
                          hipStream_t st);
// clip[0] = min(1, max_norm / (norm + 1e-6)), clip[1] = norm = gscale * sqrt(sum partial[0:total))
// with the sum, the root and the quotient in float64 and a fixed order.  A non-finite sum
// gives clip[0] = NaN.  One workgroup.
void mv_launch_clip_finalize(const float* partial, int64_t total, double gscale, double max_norm,
                             float* clip, hipStream_t st);
