// Decoder-block elementwise kernels (residual add + RMSNorm, SwiGLU, rotary position
// embedding on the grouped qkv layout) — mv_decoder.hip.  All tensors bf16 row-major unless
// noted; all arithmetic fp32; every stored value is rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// v = res + z (res == nullptr: v = z and v is not stored);  rstd = rsqrt(mean(v^2) + eps) from
// the fp32 sums;  y = v rstd w from the fp32 v.  z, res, v, y [M, H]; w [H]; rstd fp32 [M].
// H % 8 == 0, 8 <= H <= 8192, M >= 1.
void mv_rms_fwd(const void* z, const void* res, const void* w, void* v, void* y, float* rstd,
                int64_t M, int H, float eps, hipStream_t st);
// partial rows of mv_rms_bwd for M rows
int64_t mv_rms_partials(int64_t M);
// xh = v rstd, g = w dy, dv = dv_out + rstd (g - xh mean(g xh)), dw[c] = sum_rows dy xh.
// dy != nullptr; dv_out may be nullptr.  partial: fp32 [mv_rms_partials(M)][H]; dw bf16 [H]
// through mv_colsum_partials (fixed order: two runs are bit-identical).
void mv_rms_bwd(const void* dy, const void* dv_out, const void* v, const float* rstd,
                const void* w, void* dv, float* partial, void* dw, int64_t M, int H,
                hipStream_t st);

// x [M, 2 N] (a row: N gate columns, then N up columns) -> y [M, N] = silu(gate) up; N % 8 == 0
void mv_swiglu_fwd(const void* x, void* y, int64_t M, int N, hipStream_t st);
// dy [M, N], x [M, 2 N] -> dx [M, 2 N]
void mv_swiglu_bwd(const void* dy, const void* x, void* dx, int64_t M, int N, hipStream_t st);

// qkv [T, heads, 128] with T = b s tokens and heads = hq + 2 hkv -> out of the same shape: the
// first `rot` = hq + hkv heads rotated in the half-rotation pairing by the angle of table row
// pos[t] (pos == nullptr: t % s), the value heads copied.  cos, sin fp32 [P, 64].  A position
// outside [0, P) reads row 0 or P - 1, never outside the tables.  adjoint: the transposed
// rotation (sin negated), the backward of the forward.
void mv_rotary(const void* qkv, void* out, const float* cos, const float* sin, const int32_t* pos,
               int64_t T, int s, int heads, int rot, int P, bool adjoint, hipStream_t st);
