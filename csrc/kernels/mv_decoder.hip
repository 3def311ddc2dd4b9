// Decoder-block (LLaMA-style) elementwise kernels for gfx950.
//
//  * add_rms_norm    v = res + z;  y = v rsqrt(mean(v^2) + eps) w           (one pass)
//    backward        dv = dv_out + rstd (w dy - xh mean(w dy xh)), xh = v rstd: the gradient of
//                    z and of res, with the residual stream's own gradient dv_out added on the
//                    way;  dw = sum_rows dy xh                                (one pass)
//  * swiglu          y = silu(gate) up over the fused [gate | up] projection, and its backward
//  * rotary          half-rotation position embedding of the query and key heads of the grouped
//                    qkv layout, out of place; the backward is the same kernel, sin negated
//
// Row kernels (add_rms_norm) — how a row is held.  The backward needs a whole row of v and dy
// twice: once for mean(w dy xh), once for dv.  Re-reading them would make it a 6-pass kernel
// instead of 4 (dy, v, dv_out in; dv out), so the row stays on chip.  Per LANE the backward
// keeps, for each of its columns, xh and g = w dy of the current row plus w and the fp32 dw
// accumulator, which live across rows: 4 fp32 values per column, and the 2 bytes of dv_out in
// flight.  With one wave per row (the LayerNorm kernels' layout) H = 8192 is 128 columns per
// lane: 512 fp32 registers, the whole file of a wave at occupancy 1, before any address or
// temporary; packing xh and g as bf16 would still leave 128 + 128 fp32 (w, dw) + 128 packed
// = 384 and would round g and xh a second time.  Instead a row is split over WPR waves of one
// workgroup: 64 WPR lanes x 8 columns per 16-B chunk, NCH <= 4 chunks per lane, so at most 32
// columns per lane whatever H is:
//
//      H <= 512   WPR 1  NCH 1       H <= 4096  WPR 2  NCH 4
//      H <= 1024  WPR 1  NCH 2       H <= 8192  WPR 4  NCH 4
//      H <= 2048  WPR 1  NCH 4
//
// That is 4 x 32 = 128 fp32 registers of row state in the widest form (the compiler's count for
// every instantiation, all without scratch, is in docs/DECODER_BLOCK.md), and a lane issues its
// NCH loads of each operand (2 NCH forward, 3 NCH backward) before it uses the first.  The price
// is the row statistic: one float per wave through LDS and one workgroup barrier per row (two LDS
// slots used in turn, so a row needs no second barrier).  With WPR < 4 a workgroup runs 4 / WPR
// rows side by side.  A workgroup of the backward covers 32 consecutive rows and writes ONE fp32
// partial row of dw (the row groups of a workgroup combine through LDS in a fixed order);
// mv_bert's fixed-order column-sum kernel finishes: no atomics, bit-identical runs.
//
// swiglu: the 2-D geometry of bias_gelu (2048-column slabs x row ranges), two rows per step:
// 4 (forward) / 6 (backward) independent 16-B loads per lane in flight.
//
// rotary: a lane owns dims d0 .. d0 + 7 and their partners d0 + 64 .. of one (token, head):
// two 16-B loads, two 32-B table loads, two 16-B stores; the 8 lanes of a head read 2 x 128
// contiguous bytes, and the two halves meet in registers only.  Lanes of a value head store the
// 32 bytes they loaded.
#include "mv_decoder.h"
#include "mv_bert.h"
#include "mv_common.h"

namespace mv {
namespace dec {

constexpr int kBwdRows = 32;           // rows per workgroup (= per partial row) of rms_bwd

__device__ __forceinline__ void unpack8(const u16x8& a, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(((uint32_t)a[j]) << 16);
}

// Sum of s over the WPR waves of a row group (fixed order).  red: this row group's WPR floats
// of the LDS slot in turn; every wave of the workgroup reaches the barrier.
template <int WPR>
__device__ __forceinline__ float row_sum(float s, float* red) {
  s = wave_sum(s);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) % WPR] = s;
    __syncthreads();
    s = red[0];
#pragma unroll
    for (int i = 1; i < WPR; ++i) s += red[i];
  }
  return s;
}

// ------------------------------------------------------------ residual add + RMSNorm
template <int WPR, int NCH>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const __bf16* __restrict__ z,
                                                       const __bf16* __restrict__ res,
                                                       const __bf16* __restrict__ w,
                                                       __bf16* __restrict__ v,
                                                       __bf16* __restrict__ y,
                                                       float* __restrict__ rstd, int64_t M, int H,
                                                       float eps) {
  constexpr int RG = 4 / WPR, TPR = 64 * WPR;
  const int t = threadIdx.x % TPR, rg = threadIdx.x / TPR;
  const int64_t row = (int64_t)blockIdx.x * RG + rg;
  const bool live = row < M;          // no early exit: row_sum holds a workgroup barrier
  float x[NCH][8], r[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {     // every load of the row is issued before the first use
    const int c = (k * TPR + t) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[k][j] = r[k][j] = 0.f;
    if (live && c < H) {
      load8(z + row * H + c, x[k]);
      if (res) load8(res + row * H + c, r[k]);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (k * TPR + t) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[k][j] += r[k][j];
      s += x[k][j] * x[k][j];
    }
    if (res && live && c < H) store8(v + row * H + c, x[k]);
  }
  __shared__ float red[RG][WPR];
  const float rs = rsqrtf(row_sum<WPR>(s, red[rg]) / (float)H + eps);
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (k * TPR + t) * 8;
    if (live && c < H) {
      float gm[8], o[8];
      load8(w + c, gm);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = x[k][j] * rs * gm[j];
      store8(y + row * H + c, o);
    }
  }
  if (live && t == 0) rstd[row] = rs;
}

template <int WPR, int NCH>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const __bf16* __restrict__ dy,
                                                       const __bf16* __restrict__ dvo,
                                                       const __bf16* __restrict__ v,
                                                       const float* __restrict__ rstd,
                                                       const __bf16* __restrict__ w,
                                                       __bf16* __restrict__ dv,
                                                       float* __restrict__ partial, int64_t M,
                                                       int H) {
  constexpr int RG = 4 / WPR, TPR = 64 * WPR, RPG = kBwdRows / RG;
  const int t = threadIdx.x % TPR, rg = threadIdx.x / TPR;
  float gm[NCH][8], dwa[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (k * TPR + t) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) gm[k][j] = dwa[k][j] = 0.f;
    if (c < H) load8(w + c, gm[k]);                   // once per workgroup, not per row
  }
  __shared__ float red[2][RG][WPR];
  const int64_t rbeg = (int64_t)blockIdx.x * kBwdRows + rg * RPG;
  const float inv_h = 1.f / (float)H;
  for (int rr = 0; rr < RPG; ++rr) {                  // uniform trip count: barrier inside
    const int64_t row = rbeg + rr;
    const bool live = row < M;
    const float rs = live ? rstd[row] : 0.f;
    float xh[NCH][8], g[NCH][8];
    u16x8 e[NCH];                                     // dv_out, kept packed until it is added
#pragma unroll
    for (int k = 0; k < NCH; ++k) {                   // 3 NCH independent 16-B loads in flight
      const int c = (k * TPR + t) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) xh[k][j] = g[k][j] = 0.f;
      e[k] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live && c < H) {
        load8(dy + row * H + c, g[k]);
        load8(v + row * H + c, xh[k]);
        if (dvo) e[k] = *reinterpret_cast<const u16x8*>(dvo + row * H + c);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xh[k][j] *= rs;
        dwa[k][j] += g[k][j] * xh[k][j];
        g[k][j] *= gm[k][j];
        s += g[k][j] * xh[k][j];
      }
    s = row_sum<WPR>(s, red[rr & 1][rg]) * inv_h;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = (k * TPR + t) * 8;
      if (live && c < H) {
        float d[8], a[8];
        unpack8(e[k], a);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = a[j] + rs * (g[k][j] - xh[k][j] * s);
        store8(dv + row * H + c, d);
      }
    }
  }
  // this workgroup's partial row of dw: the RG row groups hold the same columns and combine
  // through LDS in a fixed order; with RG == 1 every lane owns its columns alone
  float* dst = partial + (int64_t)blockIdx.x * H;
  if constexpr (RG == 1) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = (k * TPR + t) * 8;
      if (c < H) store8(dst + c, dwa[k]);
    }
  } else {
    __shared__ float comb[RG][TPR * 8];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) comb[rg][t * 8 + j] = dwa[k][j];
      __syncthreads();
      for (int i = threadIdx.x; i < TPR * 8; i += 256) {
        const int c = k * TPR * 8 + i;
        if (c < H) {
          if constexpr (RG == 2) dst[c] = comb[0][i] + comb[1][i];
          else dst[c] = (comb[0][i] + comb[1][i]) + (comb[2][i] + comb[3][i]);
        }
      }
    }
  }
}

// ----------------------------------------------------------------------- SwiGLU
// A workgroup owns gate columns [c0, c0 + 2048) (256 lanes x 8), the up columns N further on,
// and a range of rows.
__device__ __forceinline__ float sigmoidf_fast(float g) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-g));
}

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const __bf16* __restrict__ x,
                                                          __bf16* __restrict__ y, int64_t M, int N,
                                                          int64_t rows_per_block) {
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  const int64_t ld = 2 * (int64_t)N;
  int64_t r = r0;
  for (; r + 1 < r1; r += 2) {        // 2 rows x (gate, up) = 4 loads in flight per lane
    float g[2][8], u[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      load8(x + (r + i) * ld + c, g[i]);
      load8(x + (r + i) * ld + N + c, u[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[i][j] = g[i][j] * sigmoidf_fast(g[i][j]) * u[i][j];
      store8(y + (r + i) * N + c, g[i]);
    }
  }
  if (r < r1) {
    float g[8], u[8];
    load8(x + r * ld + c, g);
    load8(x + r * ld + N + c, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = g[j] * sigmoidf_fast(g[j]) * u[j];
    store8(y + r * N + c, g);
  }
}

// d gate = dy up sig (1 + g (1 - sig)), d up = dy g sig
__device__ __forceinline__ void swiglu_grad8(const float (&dy)[8], float (&g)[8], float (&u)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sg = sigmoidf_fast(g[j]);
    const float dg = dy[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
    u[j] = dy[j] * g[j] * sg;
    g[j] = dg;
  }
}

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const __bf16* __restrict__ dy,
                                                          const __bf16* __restrict__ x,
                                                          __bf16* __restrict__ dx, int64_t M, int N,
                                                          int64_t rows_per_block) {
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  const int64_t ld = 2 * (int64_t)N;
  int64_t r = r0;
  for (; r + 1 < r1; r += 2) {        // 2 rows x (dy, gate, up) = 6 loads in flight per lane
    float d[2][8], g[2][8], u[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      load8(dy + (r + i) * N + c, d[i]);
      load8(x + (r + i) * ld + c, g[i]);
      load8(x + (r + i) * ld + N + c, u[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      swiglu_grad8(d[i], g[i], u[i]);
      store8(dx + (r + i) * ld + c, g[i]);
      store8(dx + (r + i) * ld + N + c, u[i]);
    }
  }
  if (r < r1) {
    float d[8], g[8], u[8];
    load8(dy + r * N + c, d);
    load8(x + r * ld + c, g);
    load8(x + r * ld + N + c, u);
    swiglu_grad8(d, g, u);
    store8(dx + r * ld + c, g);
    store8(dx + r * ld + N + c, u);
  }
}

// ----------------------------------------------------------------------- rotary
// One lane per (token, head, 8 dims of the low half): global lane index g = (token heads +
// head) 8 + d0 / 8.  ADJ: the transposed rotation.
template <bool ADJ>
__global__ __launch_bounds__(256) void rotary_kernel(const __bf16* __restrict__ x,
                                                      __bf16* __restrict__ out,
                                                      const float* __restrict__ cs,
                                                      const float* __restrict__ sn,
                                                      const int32_t* __restrict__ pos, int64_t T,
                                                      int s, int heads, int rot, int P) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t th = g >> 3;
  if (th >= T * heads) return;
  const int d0 = (int)(g & 7) * 8;
  const int64_t tok = th / heads;
  const int head = (int)(th - tok * heads);
  const int64_t off = th * 128 + d0;
  const u16x8 a = *reinterpret_cast<const u16x8*>(x + off);
  const u16x8 b = *reinterpret_cast<const u16x8*>(x + off + 64);
  if (head >= rot) {                  // a value head: the bits it loaded
    *reinterpret_cast<u16x8*>(out + off) = a;
    *reinterpret_cast<u16x8*>(out + off + 64) = b;
    return;
  }
  int p = pos ? pos[tok] : (int)(tok % s);
  p = p < 0 ? 0 : (p >= P ? P - 1 : p);               // never outside the tables
  float c[8], sv[8], lo[8], hi[8], olo[8], ohi[8];
  load8(cs + (int64_t)p * 64 + d0, c);
  load8(sn + (int64_t)p * 64 + d0, sv);
  unpack8(a, lo);
  unpack8(b, hi);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sj = ADJ ? -sv[j] : sv[j];
    olo[j] = lo[j] * c[j] - hi[j] * sj;
    ohi[j] = hi[j] * c[j] + lo[j] * sj;
  }
  store8(out + off, olo);
  store8(out + off + 64, ohi);
}

}  // namespace dec
}  // namespace mv

using namespace mv::dec;

void mv_rms_fwd(const void* z, const void* res, const void* w, void* v, void* y, float* rstd,
                int64_t M, int H, float eps, hipStream_t st) {
  auto go = [&](auto kern, int rows) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((M + rows - 1) / rows)), dim3(256), 0, st,
                       (const __bf16*)z, (const __bf16*)res, (const __bf16*)w, (__bf16*)v,
                       (__bf16*)y, rstd, M, H, eps);
  };
  if (H <= 512) go(rms_fwd_kernel<1, 1>, 4);
  else if (H <= 1024) go(rms_fwd_kernel<1, 2>, 4);
  else if (H <= 2048) go(rms_fwd_kernel<1, 4>, 4);
  else if (H <= 4096) go(rms_fwd_kernel<2, 4>, 2);
  else go(rms_fwd_kernel<4, 4>, 1);
}

int64_t mv_rms_partials(int64_t M) { return (M + kBwdRows - 1) / kBwdRows; }

void mv_rms_bwd(const void* dy, const void* dv_out, const void* v, const float* rstd,
                const void* w, void* dv, float* partial, void* dw, int64_t M, int H,
                hipStream_t st) {
  const int64_t P = mv_rms_partials(M);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), 0, st, (const __bf16*)dy,
                       (const __bf16*)dv_out, (const __bf16*)v, rstd, (const __bf16*)w,
                       (__bf16*)dv, partial, M, H);
  };
  if (H <= 512) go(rms_bwd_kernel<1, 1>);
  else if (H <= 1024) go(rms_bwd_kernel<1, 2>);
  else if (H <= 2048) go(rms_bwd_kernel<1, 4>);
  else if (H <= 4096) go(rms_bwd_kernel<2, 4>);
  else go(rms_bwd_kernel<4, 4>);
  mv_colsum_partials(partial, (int)P, H, dw, st);
}

// rows per workgroup for about 2048 workgroups per pass, at least 8 rows each
static int64_t swiglu_rows(int64_t M, int N, unsigned* gx) {
  const int gy = (N + 2047) / 2048;
  int64_t blocks = 2048 / gy;
  if (blocks < 1) blocks = 1;
  int64_t rpb = (M + blocks - 1) / blocks;
  if (rpb < 8) rpb = 8;
  *gx = (unsigned)((M + rpb - 1) / rpb);
  return rpb;
}

void mv_swiglu_fwd(const void* x, void* y, int64_t M, int N, hipStream_t st) {
  unsigned gx;
  const int64_t rpb = swiglu_rows(M, N, &gx);
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(gx, (N + 2047) / 2048), dim3(256), 0, st,
                     (const __bf16*)x, (__bf16*)y, M, N, rpb);
}

void mv_swiglu_bwd(const void* dy, const void* x, void* dx, int64_t M, int N, hipStream_t st) {
  unsigned gx;
  const int64_t rpb = swiglu_rows(M, N, &gx);
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(gx, (N + 2047) / 2048), dim3(256), 0, st,
                     (const __bf16*)dy, (const __bf16*)x, (__bf16*)dx, M, N, rpb);
}

void mv_rotary(const void* qkv, void* out, const float* cos, const float* sin, const int32_t* pos,
               int64_t T, int s, int heads, int rot, int P, bool adjoint, hipStream_t st) {
  const int64_t lanes = T * heads * 8;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (adjoint)
    hipLaunchKernelGGL(rotary_kernel<true>, grid, dim3(256), 0, st, (const __bf16*)qkv,
                       (__bf16*)out, cos, sin, pos, T, s, heads, rot, P);
  else
    hipLaunchKernelGGL(rotary_kernel<false>, grid, dim3(256), 0, st, (const __bf16*)qkv,
                       (__bf16*)out, cos, sin, pos, T, s, heads, rot, P);
}
