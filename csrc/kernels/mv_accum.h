// Host-side declarations of the local gradient accumulation launchers (mv_accum.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mv_kernels.h"

// Multi-tensor launches over the tensor table of mt_copy (MtArgs: tensor i of grad_dtype holds
// numel[i] elements and owns [flat_off[i], flat_off[i] + numel[i]) of the flat buffers).
//
// first: acc[off + i]  = float(g[i])      (a write: the accumulator needs no zeroing pass)
// add:   acc[off + i] += float(g[i])
void mv_launch_accumulate(const MtArgs& a, int grad_dtype, float* acc, bool first, hipStream_t st);
// last:  dst[off + i] = cast((acc[off + i] + float(g[i])) * scale), dst of wire_dtype; the fp32
// product is rounded before the cast.  acc is only read.  found_nonfinite (nullable) |= any
// stored value that is not finite, an overflow of the cast included (as mv_launch_mt_copy).
void mv_launch_pack_accumulated(const MtArgs& a, int grad_dtype, const float* acc, void* dst,
                                int wire_dtype, float scale, int* found_nonfinite,
                                hipStream_t st);
