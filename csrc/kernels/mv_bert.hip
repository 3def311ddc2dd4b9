// Fused transformer elementwise kernels (BERT) for gfx950.
//
//  * bias_gelu       y = gelu(x + b)             (x = GEMM output without bias)
//    backward        dx = dy * gelu'(x + b), dbias = sum_rows dx  (one pass)
//  * bias_dropout_add_ln
//                    v = res + dropout(z + b);  y = LN(v) * gamma + beta
//    backward        dv = LN'(dy) (the residual's grad), dz = dropout'(dv),
//                    dgamma / dbeta / dbias column sums            (one pass)
//
// Replaces, per BERT layer, torch's separate bias-add (inside the GEMM), GELU,
// dropout, residual add, LayerNorm and their backward kernels plus the
// bias-gradient reductions (profiles/r1_bert_large_fused_attention.md).
// Dropout masks come from a counter hash of (seed, row, col) — no mask tensor.
//
// Row kernels: one wave per row (wave64, 8 bf16 per lane per 512-column chunk,
// all chunks held in registers, H <= 4096, H % 512 == 0 or H % 8 == 0 with
// guards); row statistics by wave shuffles.  Column sums: each lane owns fixed
// columns across the rows its wave processes, waves combine through LDS in a
// fixed order, one partial row per workgroup, then a fixed-order finalize
// kernel — deterministic.
#include "mv_bert.h"
#include "mv_common.h"

#include <cstdlib>

namespace mv {
namespace tx {

constexpr int kRowsPerBlock = 64;      // 4 waves x 16 rows

// Dropout keep bits of columns c .. c + 7 of one row (c % 8 == 0): one mix32 per column
// PAIR (the row key + pair index, as the attention kernels' drop_pair), its low 16 bits
// deciding the even column and its high 16 bits the odd one; drop when below
// th = round(p 2^16).  Round 6: the per-element hash (two chained mix32, 32-bit threshold)
// made the LayerNorm forward / backward passes VALU-bound (ln_bwd at 69% of HBM).
__device__ __forceinline__ uint32_t keep8(uint32_t seed, uint32_t row, uint32_t c, uint32_t th) {
  const uint32_t rk = mix32(seed + row * 0x9E3779B1u);
  uint32_t m = 0u;
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const uint32_t h = mix32(rk + ((c + (uint32_t)j) >> 1) * 0x85EBCA6Bu);
    m |= ((uint32_t)((h & 0xFFFFu) >= th) << j) | ((uint32_t)((h >> 16) >= th) << (j + 1));
  }
  return m;
}

// gelu / gelu_grad: mv_common.h (shared with the 256 x 256 GEMM's GELU-backward epilogue)

// --------------------------------------------------------------- bias + GELU
// 2-D geometry: a workgroup owns columns [c0, c0 + 2048) (256 lanes x 8) and
// a range of rows; each lane keeps its 8 columns' bias and partial sums.
__global__ __launch_bounds__(256) void bias_gelu_fwd_kernel(const __bf16* __restrict__ x,
                                                             const __bf16* __restrict__ b,
                                                             __bf16* __restrict__ y, int64_t M,
                                                             int N, int64_t rows_per_block) {
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  float bv[8];
  load8(b + c, bv);
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  int64_t r = r0;
  // 4 rows per step: 4 independent 16-B loads in flight per lane (one row at a time
  // left the lane waiting on each load's full latency: ~4 TB/s)
  for (; r + 3 < r1; r += 4) {
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8(x + (r + u) * N + c, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[u][j] = gelu(v[u][j] + bv[j]);
      store8(y + (r + u) * N + c, v[u]);
    }
  }
  for (; r < r1; ++r) {
    float v[8];
    load8(x + r * N + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = gelu(v[j] + bv[j]);
    store8(y + r * N + c, v);
  }
}

__global__ __launch_bounds__(256) void bias_gelu_bwd_kernel(const __bf16* __restrict__ dy,
                                                             const __bf16* __restrict__ x,
                                                             const __bf16* __restrict__ b,
                                                             __bf16* __restrict__ dx,
                                                             float* __restrict__ partial,
                                                             int64_t M, int N,
                                                             int64_t rows_per_block) {
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  float bv[8], acc[8];
  load8(b + c, bv);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  int64_t r = r0;
  for (; r + 1 < r1; r += 2) {   // 2 rows x 2 tensors = 4 loads in flight per lane
    float v[2][8], g[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      load8(x + (r + u) * N + c, v[u]);
      load8(dy + (r + u) * N + c, g[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[u][j] *= gelu_grad(v[u][j] + bv[j]);
        acc[j] += g[u][j];
      }
      store8(dx + (r + u) * N + c, g[u]);
    }
  }
  for (; r < r1; ++r) {
    float v[8], g[8];
    load8(x + r * N + c, v);
    load8(dy + r * N + c, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] *= gelu_grad(v[j] + bv[j]);
      acc[j] += g[j];
    }
    store8(dx + r * N + c, g);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) partial[(int64_t)blockIdx.x * N + c + j] = acc[j];
}

// Column-sum partials of a bf16 [M, N] matrix (a linear layer's bias gradient, sum over
// tokens of dy): the bias_gelu geometry, 4 rows x 16 B in flight per lane, fp32 partial
// row per row block; colsum_kernel finishes in a fixed order (deterministic).
__global__ __launch_bounds__(256) void rowsum_partial_kernel(const __bf16* __restrict__ dy,
                                                              float* __restrict__ partial,
                                                              int64_t M, int N,
                                                              int64_t rows_per_block) {
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8(dy + (r + u) * N + c, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[u][j];
  }
  for (; r < r1; ++r) {
    float v[8];
    load8(dy + r * N + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) partial[(int64_t)blockIdx.x * N + c + j] = acc[j];
}

// The same for an even N that is not a multiple of 8 (BERT's 30,522-word MLM decoder bias):
// rows are only 4-byte aligned, so a lane sums 2 columns (4-byte loads, 4 rows in flight);
// a workgroup covers 512 columns of one row block.
__global__ __launch_bounds__(256) void rowsum_partial2_kernel(const __bf16* __restrict__ dy,
                                                               float* __restrict__ partial,
                                                               int64_t M, int N,
                                                               int64_t rows_per_block) {
  const int c = blockIdx.y * 512 + threadIdx.x * 2;
  if (c >= N) return;
  float a0 = 0.f, a1 = 0.f;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const uint32_t*>(dy + (r + u) * N + c);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a0 += __uint_as_float(v[u] << 16);
      a1 += __uint_as_float(v[u] & 0xffff0000u);
    }
  }
  for (; r < r1; ++r) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(dy + r * N + c);
    a0 += __uint_as_float(v << 16);
    a1 += __uint_as_float(v & 0xffff0000u);
  }
  partial[(int64_t)blockIdx.x * N + c] = a0;
  partial[(int64_t)blockIdx.x * N + c + 1] = a1;
}

// Column sums of fp32 partials -> bf16.  Partial row p of set `y` lives at
// partial + y*set_off + p*stride.  A workgroup owns 16 columns x 16 row groups
// (64 B coalesced per row, >= 192 workgroups for BERT's shapes); the 16 group
// sums combine through LDS in a fixed order: deterministic.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ partial, int P,
                                                      int N, int64_t stride, int64_t set_off,
                                                      __bf16* __restrict__ out0,
                                                      __bf16* __restrict__ out1,
                                                      __bf16* __restrict__ out2) {
  __bf16* out = blockIdx.y == 0 ? out0 : (blockIdx.y == 1 ? out1 : out2);
  if (!out) return;                                    // uniform per workgroup
  const int tc = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + tc;
  const float* base = partial + blockIdx.y * set_off + c;
  // 8 independent partial rows in flight per lane (the pass is latency-bound: ~200
  // workgroups over up to 1,024 partial rows)
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < N) {
    int p = g;
    for (; p + 112 < P; p += 128) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = base[(int64_t)(p + 16 * u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += v[u];
    }
    for (; p < P; p += 16) a[0] += base[(int64_t)p * stride];
  }
  __shared__ float red[16][17];
  red[g][tc] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (g == 0 && c < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][tc];
    out[c] = (__bf16)t;
  }
}

// ------------------------------------------------- bias + dropout + add + LN
struct LnArgs {
  const __bf16* z;      // [M, H] GEMM output (no bias)
  const __bf16* bias;   // [H] or null
  const __bf16* res;    // [M, H] residual or null
  const __bf16* gamma;  // [H]
  const __bf16* beta;   // [H]
  __bf16* v;            // [M, H] saved pre-LN sum
  __bf16* y;            // [M, H]
  float* mean;          // [M]
  float* rstd;          // [M]
  int64_t M;
  int H;
  float eps;
  float p_drop;
  uint32_t seed;
  uint32_t thresh;
};

template <int NCH>
__global__ __launch_bounds__(256) void ln_fwd_kernel(LnArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const float inv_keep = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;
  float v[NCH][8];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = k * 512 + lane * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
    if (c < a.H) {
      float z[8], bb[8], rr[8];
      load8(a.z + row * a.H + c, z);
      if (a.bias) load8(a.bias + c, bb);
      if (a.res) load8(a.res + row * a.H + c, rr);
      const uint32_t km = a.p_drop > 0.f ? keep8(a.seed, (uint32_t)row, (uint32_t)c, a.thresh) : ~0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = z[j] + (a.bias ? bb[j] : 0.f);
        if (a.p_drop > 0.f) t = ((km >> j) & 1u) ? t * inv_keep : 0.f;
        t += a.res ? rr[j] : 0.f;
        v[k][j] = (float)(__bf16)t;     // stats on the stored (bf16) value
        s += v[k][j];
      }
      if (a.v) store8(a.v + row * a.H + c, v[k]);
    }
  }
  const float mean = wave_sum(s) / (float)a.H;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    if (k * 512 + lane * 8 < a.H) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[k][j] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)a.H + a.eps);
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = k * 512 + lane * 8;
    if (c < a.H) {
      float gm[8], bt[8], o[8];
      load8(a.gamma + c, gm);
      load8(a.beta + c, bt);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[k][j] - mean) * rstd * gm[j] + bt[j];
      store8(a.y + row * a.H + c, o);
    }
  }
  if (lane == 0) {
    a.mean[row] = mean;
    a.rstd[row] = rstd;
  }
}

struct LnBwdArgs {
  const __bf16* dy;     // [M, H]
  const __bf16* v;      // [M, H] saved pre-LN sum
  const float* mean;    // [M]
  const float* rstd;    // [M]
  const __bf16* gamma;  // [H]
  __bf16* dv;           // [M, H] grad of the sum (= residual grad)
  __bf16* dz;           // [M, H] grad of z (dropout backward), or null
  float* partial;       // [P][3][H]: dgamma, dbeta, dbias(= sum dz)
  int64_t M;
  int H;
  float p_drop;
  uint32_t seed;
  uint32_t thresh;
  const __bf16* dy2;    // [M, H] second gradient stream of y, added on load, or null
};

// Write one wave-partial set (this wave's 8 x NCH columns) into LDS slot w, then
// combine the 4 waves in fixed order into partial row `which` of this block.
template <int NCH>
__device__ __forceinline__ void block_colsum(const float (&src)[NCH][8], float (*red)[512],
                                             float* __restrict__ dst, int H) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][lane * 8 + j] = src[k][j];
    __syncthreads();
    for (int t = threadIdx.x; t < 512; t += 256) {
      const int c = k * 512 + t;
      if (c < H) dst[c] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
  }
}

template <int NCH>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdArgs a) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inv_keep = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;
  float dg[NCH][8], db[NCH][8], dzs[NCH][8], gm[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = k * 512 + lane * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) dg[k][j] = db[k][j] = dzs[k][j] = gm[k][j] = 0.f;
    if (c < a.H) load8(a.gamma + c, gm[k]);       // once per kernel, not per row
  }
  // the next row's dy / dy2 / v are loaded (raw 16-byte vectors) while the current
  // row is reduced and written: a wave keeps two rows of loads in flight instead of
  // waiting a full memory latency at the top of every row
  struct Raw {
    u32x4 dy[NCH], d2[NCH], v[NCH];
    float mu, rs;         // the row's saved statistics travel with its prefetch (loaded at
                          // the top of the row they cost one dependent round trip per row)
  };
  auto ld = [&](int64_t row, Raw& R) {
    const int64_t rc = row < a.M ? row : a.M - 1;
    R.mu = a.mean[rc];
    R.rs = a.rstd[rc];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = k * 512 + lane * 8;
      R.dy[k] = R.d2[k] = R.v[k] = u32x4{0u, 0u, 0u, 0u};
      if (c < a.H && row < a.M) {
        R.dy[k] = *reinterpret_cast<const u32x4*>(a.dy + row * a.H + c);
        if (a.dy2) R.d2[k] = *reinterpret_cast<const u32x4*>(a.dy2 + row * a.H + c);
        R.v[k] = *reinterpret_cast<const u32x4*>(a.v + row * a.H + c);
      }
    }
  };
  auto unpack = [](const u32x4& r, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = __uint_as_float(r[j] << 16);
      o[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
    }
  };
  const int64_t rbeg = (int64_t)blockIdx.x * kRowsPerBlock + w * (kRowsPerBlock / 4);
  constexpr bool PF = NCH <= 2;         // wider rows: no room for a second row of loads
  Raw cur, nxt;
  if (PF) ld(rbeg, cur);
  for (int rr = 0; rr < kRowsPerBlock / 4; ++rr) {
    const int64_t row = rbeg + rr;
    if (row >= a.M) break;
    if (!PF) ld(row, cur);
    else if (rr + 1 < kRowsPerBlock / 4) ld(row + 1, nxt);
    const float mean = cur.mu, rstd = cur.rs;
    float xh[NCH][8], g[NCH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = k * 512 + lane * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) xh[k][j] = g[k][j] = 0.f;
      if (c < a.H) {
        float dy[8], vv[8];
        unpack(cur.dy[k], dy);
        if (a.dy2) {   // residual use of y (mivod.ops.bn.tap): no separate autograd add
          float e[8];
          unpack(cur.d2[k], e);
#pragma unroll
          for (int j = 0; j < 8; ++j) dy[j] += e[j];
        }
        unpack(cur.v[k], vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[k][j] = (vv[j] - mean) * rstd;
          g[k][j] = dy[j] * gm[k][j];
          s1 += g[k][j];
          s2 += g[k][j] * xh[k][j];
          dg[k][j] += dy[j] * xh[k][j];
          db[k][j] += dy[j];
        }
      }
    }
    s1 = wave_sum(s1) / (float)a.H;
    s2 = wave_sum(s2) / (float)a.H;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = k * 512 + lane * 8;
      if (c < a.H) {
        float d[8], z[8];
        const uint32_t km = a.p_drop > 0.f ? keep8(a.seed, (uint32_t)row, (uint32_t)c, a.thresh) : ~0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          d[j] = rstd * (g[k][j] - s1 - xh[k][j] * s2);
          float t = d[j];
          if (a.p_drop > 0.f) t = ((km >> j) & 1u) ? t * inv_keep : 0.f;
          z[j] = t;
          dzs[k][j] += t;
        }
        store8(a.dv + row * a.H + c, d);
        if (a.dz) store8(a.dz + row * a.H + c, z);
      }
    }
    if (PF) cur = nxt;
  }
  __shared__ float red[4][512];
  float* base = a.partial + (int64_t)blockIdx.x * 3 * a.H;
  block_colsum<NCH>(dg, red, base, a.H);
  block_colsum<NCH>(db, red, base + a.H, a.H);
  block_colsum<NCH>(dzs, red, base + 2 * a.H, a.H);
}

// ------------------------------------------------ cross entropy over bf16 logits
// BERT's MLM head: logits [R, V] bf16 (V even), one workgroup per row.  Forward: an online
// (max, sum exp) per lane over bf16 pairs, combined across the workgroup; lse[r] and
// loss[r] = lse - x[r, label] (0 for an ignored row) in fp32.  Backward: dlogits =
// scale * (exp(x - lse) - onehot(label)) written as bf16 in the same pass over x (0 rows
// for ignored labels); scale = upstream gradient / valid rows, read from device memory.
// Replaces the fp32 copy of the logits, softmax forward / backward and the bf16 cast of
// the gradient (torch's F.cross_entropy on logits.float()).
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - mm)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mm));
  m = mm;
}

__global__ __launch_bounds__(256) void ce_fwd_kernel(const __bf16* __restrict__ x,
                                                      const int64_t* __restrict__ labels,
                                                      int V, int64_t ignore,
                                                      float* __restrict__ lse,
                                                      float* __restrict__ loss) {
  const int64_t r = blockIdx.x;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(x + r * V);
  const int np = V >> 1;
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) {
    const uint32_t u = row[i];
    const float a = __uint_as_float(u << 16), b = __uint_as_float(u & 0xffff0000u);
    const float mx = fmaxf(a, b);
    if (mx > m) {
      s = (m == -INFINITY ? 0.f : s * __expf(m - mx));
      m = mx;
    }
    s += __expf(a - m) + __expf(b - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, kWave), s2 = __shfl_xor(s, o, kWave);
    lse_merge(m, s, m2, s2);
  }
  __shared__ float red[2][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = m;
    red[1][w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mm = red[0][0], ss = red[1][0];
    for (int k = 1; k < 4; ++k) lse_merge(mm, ss, red[0][k], red[1][k]);
    const float l = mm + __logf(ss);
    lse[r] = l;
    const int64_t lab = labels[r];
    float v = 0.f;
    if (lab != ignore && lab >= 0 && lab < V) v = l - (float)x[r * V + lab];
    loss[r] = v;
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const __bf16* __restrict__ x,
                                                      const int64_t* __restrict__ labels,
                                                      const float* __restrict__ lse,
                                                      const float* __restrict__ scale, int V,
                                                      int64_t ignore, __bf16* __restrict__ dx) {
  const int64_t r = blockIdx.x;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(x + r * V);
  uint32_t* out = reinterpret_cast<uint32_t*>(dx + r * V);
  const int np = V >> 1;
  const int64_t lab = labels[r];
  const bool valid = lab != ignore && lab >= 0 && lab < V;
  const float g = valid ? scale[0] : 0.f, l = lse[r];
  for (int i = threadIdx.x; i < np; i += 256) {
    const uint32_t u = row[i];
    float a = __uint_as_float(u << 16), b = __uint_as_float(u & 0xffff0000u);
    a = __expf(a - l);
    b = __expf(b - l);
    if (2 * i == lab) a -= 1.f;
    if (2 * i + 1 == lab) b -= 1.f;
    out[i] = cvt_pk_bf16(g * a, g * b);
  }
}

}  // namespace tx
}  // namespace mv

using namespace mv::tx;

void mv_ce_fwd(const void* x, const int64_t* labels, int64_t R, int V, int64_t ignore, float* lse,
               float* loss, hipStream_t st) {
  hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)R), dim3(256), 0, st, (const __bf16*)x, labels,
                     V, ignore, lse, loss);
}

void mv_ce_bwd(const void* x, const int64_t* labels, const float* lse, const float* scale,
               int64_t R, int V, int64_t ignore, void* dx, hipStream_t st) {
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)R), dim3(256), 0, st, (const __bf16*)x, labels,
                     lse, scale, V, ignore, (__bf16*)dx);
}

static int64_t rows_per_block_for(int64_t M, int N, int64_t* P) {
  const int gy = (N + 2047) / 2048;
  constexpr int64_t total = 2048;        // workgroups per pass
  int64_t blocks = total / gy;
  if (blocks < 1) blocks = 1;
  int64_t rpb = (M + blocks - 1) / blocks;
  if (rpb < 8) rpb = 8;
  *P = (M + rpb - 1) / rpb;
  return rpb;
}

int64_t mv_bias_gelu_partials(int64_t M, int N) {
  int64_t P;
  rows_per_block_for(M, N, &P);
  return P;
}

namespace mv {
namespace tx {

// Embedding backward (word embeddings: T tokens -> V rows): the token rows sorted by id
// (sid, perm from a stable sort), ONE workgroup per sorted position; the workgroup at the
// first row of a run of equal ids sums the run's dy rows in sorted (= token) order in fp32
// and writes that id's gradient row once; the others exit.  Deterministic, no atomics, no
// host sync; rows of ids absent from the batch are zeroed by the caller.  (Replaces
// PyTorch's sort / segment-offset / compute_grad_weight / sum_and_scatter chain: ~0.6 ms
// per BERT-Large step.)  A run is summed by one workgroup: ~2 rows per id on uniform ids,
// batch-many for a [CLS]-like id.
__global__ __launch_bounds__(128) void emb_bwd_kernel(const __bf16* __restrict__ dy,
                                                       const int64_t* __restrict__ sid,
                                                       const int64_t* __restrict__ perm,
                                                       int64_t T, int H,
                                                       __bf16* __restrict__ dw) {
  const int64_t r0 = blockIdx.x;
  const int64_t id = sid[r0];
  if (r0 > 0 && sid[r0 - 1] == id) return;      // not the first row of its run
  int64_t r1 = r0 + 1;
  while (r1 < T && sid[r1] == id) ++r1;
  for (int c = threadIdx.x * 8; c < H; c += 128 * 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t r = r0;
    for (; r + 3 < r1; r += 4) {               // 4 rows in flight
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) load8(dy + perm[r + u] * H + c, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[u][j];
    }
    for (; r < r1; ++r) {
      float v[8];
      load8(dy + perm[r] * H + c, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
    store8(dw + id * H + c, acc);
  }
}

// BERT embedding sum y[r] = word[ids[r]] + pos[r % s] + type[tt[r]] (fp32 sum, one bf16
// rounding; PyTorch's lookup path is gather + 2 broadcast adds = 4 passes over [T, H]).
// One lane = 8 columns (16 B) of one token.  An id outside [0, V) or a type outside
// [0, ntype) reads nothing: the row is written as NaN and *bad is set (plain store of 1 from
// every offending lane), which the caller turns into a device-side assert.
__global__ __launch_bounds__(256) void bert_emb_fwd_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
    const __bf16* __restrict__ ww, const __bf16* __restrict__ wp,
    const __bf16* __restrict__ wt, __bf16* __restrict__ y, int* __restrict__ bad, int64_t T,
    int s, int H, int64_t V, int ntype) {
  const int lanes = H >> 3;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = g / lanes;
  if (r >= T) return;
  const int c = (int)(g - r * lanes) * 8;
  const int64_t id = ids[r], ty = tt[r];
  float a[8];
  if (id < 0 || id >= V || ty < 0 || ty >= ntype) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = __builtin_nanf("");
    *bad = 1;
  } else {
    float b[8], t[8];
    load8(ww + id * H + c, a);
    load8(wp + (r % s) * H + c, b);
    load8(wt + ty * H + c, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (a[j] + b[j]) + t[j];
  }
  store8(y + r * H + c, a);
}

// Position + token-type gradients of the BERT embedding sum, pass 1: dy viewed as
// [B, s H]; row block p of the batch x 2048 columns per workgroup (the bias-gradient
// geometry, 4 rows x 16 B in flight per lane); per column the sums over the block's rows
// split by the token's type (0 / 1): partial[t][p][c].
__global__ __launch_bounds__(256) void emb_pt_partial_kernel(const __bf16* __restrict__ dy,
                                                             const int64_t* __restrict__ tt,
                                                             float* __restrict__ partial,
                                                             int64_t B, int s, int H,
                                                             int64_t rows_per_block, int64_t P) {
  const int N = s * H;
  const int c = blockIdx.y * 2048 + threadIdx.x * 8;
  if (c >= N) return;
  const int si = c / H;
  float a0[8], a1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a0[j] = a1[j] = 0.f;
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < B ? r0 + rows_per_block : B;
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    float v[4][8];
    bool one[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      load8(dy + (r + u) * N + c, v[u]);
      one[u] = tt[(r + u) * s + si] != 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a0[j] += one[u] ? 0.f : v[u][j];
        a1[j] += one[u] ? v[u][j] : 0.f;
      }
  }
  for (; r < r1; ++r) {
    float v[8];
    load8(dy + r * N + c, v);
    const bool one = tt[r * s + si] != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a0[j] += one ? 0.f : v[j];
      a1[j] += one ? v[j] : 0.f;
    }
  }
  float* p0 = partial + (int64_t)blockIdx.x * N + c;
  float* p1 = p0 + P * N;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    p0[j] = a0[j];
    p1[j] = a1[j];
  }
}

// Pass 2: per column of s H the fixed-order sums S_t over the P partial rows; the position
// gradient is bf16(S_0 + S_1), S_t (fp32 [2][s H]) feeds the token-type column sums.
__global__ __launch_bounds__(256) void emb_pt_finish_kernel(const float* __restrict__ partial,
                                                            int64_t P, int N,
                                                            __bf16* __restrict__ dwp,
                                                            float* __restrict__ ts) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float s0 = 0.f, s1 = 0.f;
  for (int64_t p = 0; p < P; ++p) {
    s0 += partial[p * N + c];
    s1 += partial[(P + p) * N + c];
  }
  dwp[c] = (__bf16)(s0 + s1);
  ts[c] = s0;
  ts[N + c] = s1;
}

}  // namespace tx
}  // namespace mv

void mv_bert_emb_fwd(const int64_t* ids, const int64_t* tt, const void* ww, const void* wp,
                     const void* wt, void* y, int* bad, int64_t T, int s, int H, int64_t V,
                     int ntype, hipStream_t st) {
  if (T <= 0) return;
  const int64_t lanes = T * (H / 8);
  hipLaunchKernelGGL(mv::tx::bert_emb_fwd_kernel, dim3((unsigned)((lanes + 255) / 256)),
                     dim3(256), 0, st, ids, tt, (const __bf16*)ww, (const __bf16*)wp,
                     (const __bf16*)wt, (__bf16*)y, bad, T, s, H, V, ntype);
}

int64_t mv_emb_pt_partials(int64_t B, int s, int H) {
  int64_t P;
  rows_per_block_for(B, s * H, &P);
  return P;
}

void mv_emb_pt_bwd(const void* dy, const int64_t* tt, float* partial, float* ts, void* dwp,
                   void* dwt, int64_t B, int s, int H, hipStream_t st) {
  const int N = s * H;
  int64_t P;
  const int64_t rpb = rows_per_block_for(B, N, &P);
  hipLaunchKernelGGL(mv::tx::emb_pt_partial_kernel, dim3((unsigned)P, (N + 2047) / 2048),
                     dim3(256), 0, st, (const __bf16*)dy, tt, partial, B, s, H, rpb, P);
  hipLaunchKernelGGL(mv::tx::emb_pt_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, st,
                     (const float*)partial, P, N, (__bf16*)dwp, ts);
  // token-type rows: column sums of S_0 / S_1 viewed as [s, H] (fixed order)
  __bf16* t0 = (__bf16*)dwt;
  hipLaunchKernelGGL(colsum_kernel, dim3((H + 15) / 16, 2), dim3(256), 0, st, (const float*)ts,
                     s, H, (int64_t)H, (int64_t)N, t0, t0 + H, (__bf16*)nullptr);
}

void mv_embedding_bwd(const void* dy, const int64_t* sid, const int64_t* perm, int64_t T, int H,
                      void* dw, hipStream_t st) {
  if (T <= 0) return;
  hipLaunchKernelGGL(mv::tx::emb_bwd_kernel, dim3((unsigned)T), dim3(128), 0, st,
                     (const __bf16*)dy, sid, perm, T, H, (__bf16*)dw);
}

void mv_bias_gelu_fwd(const void* x, const void* b, void* y, int64_t M, int N, hipStream_t st) {
  int64_t P;
  const int64_t rpb = rows_per_block_for(M, N, &P);
  hipLaunchKernelGGL(bias_gelu_fwd_kernel, dim3((unsigned)P, (N + 2047) / 2048), dim3(256), 0, st,
                     (const __bf16*)x, (const __bf16*)b, (__bf16*)y, M, N, rpb);
}

void mv_bias_gelu_bwd(const void* dy, const void* x, const void* b, void* dx, float* partial,
                      void* dbias, int64_t M, int N, hipStream_t st) {
  int64_t P;
  const int64_t rpb = rows_per_block_for(M, N, &P);
  hipLaunchKernelGGL(bias_gelu_bwd_kernel, dim3((unsigned)P, (N + 2047) / 2048), dim3(256), 0, st,
                     (const __bf16*)dy, (const __bf16*)x, (const __bf16*)b, (__bf16*)dx, partial,
                     M, N, rpb);
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16, 1), dim3(256), 0, st,
                     (const float*)partial, (int)P, N, (int64_t)N, (int64_t)0, (__bf16*)dbias,
                     (__bf16*)nullptr, (__bf16*)nullptr);
}

void mv_colsum_partials(const float* partial, int P, int N, void* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16, 1), dim3(256), 0, st, partial, P, N,
                     (int64_t)N, (int64_t)0, (__bf16*)out, (__bf16*)nullptr, (__bf16*)nullptr);
}

void mv_bias_grad(const void* dy, float* partial, void* db, int64_t M, int N, hipStream_t st) {
  int64_t P;
  const int64_t rpb = rows_per_block_for(M, N, &P);
  hipLaunchKernelGGL(rowsum_partial_kernel, dim3((unsigned)P, (N + 2047) / 2048), dim3(256), 0, st,
                     (const __bf16*)dy, partial, M, N, rpb);
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16, 1), dim3(256), 0, st,
                     (const float*)partial, (int)P, N, (int64_t)N, (int64_t)0, (__bf16*)db,
                     (__bf16*)nullptr, (__bf16*)nullptr);
}

int64_t mv_bias_grad2_partials(int64_t M, int N) {
  const int64_t gy = (N + 511) / 512;
  int64_t blocks = 2048 / gy;
  if (blocks < 1) blocks = 1;
  int64_t rpb = (M + blocks - 1) / blocks;
  if (rpb < 8) rpb = 8;
  return (M + rpb - 1) / rpb;
}

void mv_bias_grad2(const void* dy, float* partial, void* db, int64_t M, int N, hipStream_t st) {
  const int64_t P = mv_bias_grad2_partials(M, N);
  const int64_t rpb = (M + P - 1) / P;
  hipLaunchKernelGGL(rowsum_partial2_kernel, dim3((unsigned)P, (N + 511) / 512), dim3(256), 0, st,
                     (const __bf16*)dy, partial, M, N, rpb);
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16, 1), dim3(256), 0, st,
                     (const float*)partial, (int)P, N, (int64_t)N, (int64_t)0, (__bf16*)db,
                     (__bf16*)nullptr, (__bf16*)nullptr);
}

void mv_colsum_bf16(const float* partial, int P, int N, int64_t stride, void* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16, 1), dim3(256), 0, st, partial, P, N,
                     stride, (int64_t)0, (__bf16*)out, (__bf16*)nullptr, (__bf16*)nullptr);
}

int64_t mv_ln_partials(int64_t M) { return (M + kRowsPerBlock - 1) / kRowsPerBlock; }

void mv_ln_fwd(const LnFwdParams& p, hipStream_t st) {
  LnArgs a{(const __bf16*)p.z, (const __bf16*)p.bias, (const __bf16*)p.res,
           (const __bf16*)p.gamma, (const __bf16*)p.beta, (__bf16*)p.v, (__bf16*)p.y, p.mean,
           p.rstd, p.M, p.H, p.eps, p.p_drop, p.seed, p.thresh};
  const dim3 g((unsigned)((p.M + 3) / 4));
  if (p.H <= 512) hipLaunchKernelGGL(ln_fwd_kernel<1>, g, dim3(256), 0, st, a);
  else if (p.H <= 1024) hipLaunchKernelGGL(ln_fwd_kernel<2>, g, dim3(256), 0, st, a);
  else if (p.H <= 2048) hipLaunchKernelGGL(ln_fwd_kernel<4>, g, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ln_fwd_kernel<8>, g, dim3(256), 0, st, a);
}

void mv_ln_bwd(const LnBwdParams& p, void* dgamma, void* dbeta, void* dbias, hipStream_t st) {
  LnBwdArgs a{(const __bf16*)p.dy, (const __bf16*)p.v, p.mean, p.rstd, (const __bf16*)p.gamma,
              (__bf16*)p.dv, (__bf16*)p.dz, p.partial, p.M, p.H, p.p_drop, p.seed, p.thresh,
              (const __bf16*)p.dy2};
  const int64_t P = mv_ln_partials(p.M);
  const dim3 g((unsigned)P);
  if (p.H <= 512) hipLaunchKernelGGL(ln_bwd_kernel<1>, g, dim3(256), 0, st, a);
  else if (p.H <= 1024) hipLaunchKernelGGL(ln_bwd_kernel<2>, g, dim3(256), 0, st, a);
  else if (p.H <= 2048) hipLaunchKernelGGL(ln_bwd_kernel<4>, g, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ln_bwd_kernel<8>, g, dim3(256), 0, st, a);
  // partial layout [P][3][H]: set stride H, row stride 3H; one launch for all three
  hipLaunchKernelGGL(colsum_kernel, dim3((p.H + 15) / 16, 3), dim3(256), 0, st,
                     (const float*)p.partial, (int)P, p.H, (int64_t)3 * p.H, (int64_t)p.H,
                     (__bf16*)dgamma, (__bf16*)dbeta, (__bf16*)dbias);
}
