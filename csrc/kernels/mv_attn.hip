// Fused multi-head attention (forward + backward) for BERT on gfx950 MFMA.
//
// Shapes: qkv [b, s, 3, h, 64] bf16 (the fused QKV projection), out [b, s, h, 64]
// bf16, optional additive key bias [b, s] fp32, attention-probability dropout.
// Head dim is fixed at 64 (BERT base/large).  All products run on
// v_mfma_f32_16x16x32_bf16 (wave64; lane l holds A[l&15][8(l>>4)+j],
// B[8(l>>4)+j][l&15], C/D row (l>>4)*4+r, col l&15).
//
// The k-major operands (V^T, Q^T, dO^T, K^T) are read from row-major LDS images with
// gfx950's transposed LDS read (ds_read_b64_tr_b16, tr8 below): no element-wise
// transposed LDS copies.
//
// Forward (one workgroup = 4 waves = 64 queries of one (b, h)): each wave keeps
// its 16 query rows as MFMA B fragments, streams K / V^T blocks of 64 keys
// through LDS, computes S^T = K Q^T so that every lane owns ONE query column
// (softmax max/sum reduce with two xor-shuffles), keeps the running max / sum
// online (exp2 domain), and feeds P straight from the accumulators into P.V as
// the A operand — the MFMA k order is permuted (keys 4g+r of two 16-key tiles)
// and V^T is read from LDS in that same order, so no transpose is needed.
// The log-sum-exp per query is saved for the backward pass.
//
// Backward (FlashAttention-2 style, one workgroup per 64-key block): each wave
// keeps K and V fragments of its 16 keys in registers, recomputes P from the
// saved LSE for every 64-query block, and accumulates dV^T += dO^T Z and
// dK^T += Q^T dS with the accumulator-as-operand trick (products that sum over
// the query = row index of the S tile need no data movement); dQ = dS K sums
// over keys, so dS goes through LDS once and each key block writes its own fp32
// dQ partial (plain stores, no atomics: deterministic), reduced by a small
// kernel — or, for s <= 128, bwd_short_kernel: one 8-wave workgroup per (b, h)
// covering every key, dQ written once in bf16 and delta computed in-kernel.
// Dropout masks are regenerated from a counter hash of
// (seed, b*h, query, key) in both passes.
#include "mv_mfma.h"
#include "mv_attn.h"


namespace mv {
namespace attn {

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr int D = 64;
constexpr int KB = 64;     // keys per block
constexpr int QB = 64;     // queries per block
constexpr int PAD = 8;     // LDS row padding (elements): 144-B rows spread banks
constexpr float LOG2E = 1.4426950408889634f;

// Counter-based dropout decision, identical in forward and backward.  One hash per PAIR
// of keys (2j, 2j + 1) of a query: 32 bits of mix32 (a bijection) of the (b, h) key xor
// the counter (q << 15 | j) — distinct for every (q, key pair) while s <= 65536 — give
// two 16-bit uniforms, the low half deciding key 2j and the high half key 2j + 1; drop
// when below thresh = round(p 2^16) (p resolution 1.5e-5).  Round 6: the previous form
// (three chained mix32 per element, 32-bit threshold) cost 55 of the forward's 215 us and
// 37 of the backward's 374 us per BERT-Large layer (scripts/micro_attn.py, p 0.1 vs 0).
__device__ __forceinline__ uint32_t drop_key(uint32_t seed, uint32_t bh) {
  return mix32(seed + bh * 0x9E3779B1u);
}
__device__ __forceinline__ uint32_t drop_pair(uint32_t dkey, uint32_t q, uint32_t k) {
  return mix32(dkey ^ ((q << 15) | (k >> 1)));
}
__device__ __forceinline__ bool drop_keep(uint32_t pair_hash, uint32_t k, uint32_t thresh) {
  return ((k & 1u) ? (pair_hash >> 16) : (pair_hash & 0xFFFFu)) >= thresh;
}
__device__ __forceinline__ bool keep_elem(uint32_t dkey, uint32_t q, uint32_t k,
                                          uint32_t thresh) {
  return drop_keep(drop_pair(dkey, q, k), k, thresh);
}

__device__ __forceinline__ unsigned short bf16_bits(float x) {
  return __builtin_bit_cast(unsigned short, (__bf16)x);
}

__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
  bf16x8 o;
  uint32_t* w = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = cvt_pk_bf16(v[2 * i], v[2 * i + 1]);
  return o;
}

__device__ __forceinline__ bf16x8 ld_b128(const __bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

// mv_mfma.h's transposed LDS read on an unswizzled row-major image of `stride` elements
// per row: lane c receives column col0 + c of rows r0 .. r0 + 3
__device__ __forceinline__ s16x4 tr4(const __bf16* base, int stride, int r0, int col0, int c) {
  return lds_tr4(base + (r0 + (c >> 2)) * stride + col0 + 4 * (c & 3));
}

// 8 k-values: rows ra .. ra+3 then rb .. rb+3 of column col0 + c
__device__ __forceinline__ bf16x8 tr8(const __bf16* base, int stride, int ra, int rb, int col0,
                                      int c) {
  const s16x4 a = tr4(base, stride, ra, col0, c);
  const s16x4 b = tr4(base, stride, rb, col0, c);
  return cat8_shuffle(a, b);
}

// Ks image of bwd_short_kernel: 128-B rows (no padding) with the 16-B chunk of column
// `col` stored at chunk (col / 8) ^ ks_swz(row), mv_mfma.h's tr_swz8 (padded rows left the
// transposed dQ reads 2-way conflicted)
__device__ __forceinline__ int ks_swz(int row) { return tr_swz8(row); }
__device__ __forceinline__ int ks_off(int row, int col) {
  return row * D + ((((col >> 3) ^ ks_swz(row)) << 3) | (col & 7));
}
// transposed read of 8 k-values of Ks for the dQ product: rows r .. r + 3 and r + 4 .. r + 7
// (r = 32 ks + 8 g) of column 16 n + c, from the lane's precomputed base of tile n (the row
// term c / 4 + 8 g and the chunk XOR are lane constants: ks_swz(32 ks + 8 g + c / 4 (+ 4))
// = c / 4 | (g & 1) << 2 for every ks)
__device__ __forceinline__ const __bf16* ks_base(const __bf16* ks, int n, int g, int c) {
  return ks + ks_off(8 * g + (c >> 2), 16 * n + 4 * (c & 3));
}
__device__ __forceinline__ bf16x8 tr8_ks(const __bf16* base_n, int ks) {
  const s16x4 a = lds_tr4(base_n + 32 * ks * D);
  const s16x4 b = lds_tr4(base_n + (32 * ks + 4) * D);
  return cat8_shuffle(a, b);
}

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
  uint32_t* w = reinterpret_cast<uint32_t*>(&z);
  w[0] = w[1] = w[2] = w[3] = 0u;
  return z;
}

// Diagnostic builds only (scripts/debug/attn_exp_probe.hip): MV_ATTN_RAW_EXP = 1 uses the raw
// v_exp_f32 builtin in the short forward's softmax; MV_ATTN_PROBE prints one query row's
// softmax state.  The shipped module is built with neither.
#ifndef MV_ATTN_RAW_EXP
#define MV_ATTN_RAW_EXP 0
#endif
#ifdef MV_ATTN_PROBE
__device__ int g_probe_bh = -1, g_probe_q = -1;
#endif

// ---------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void fwd_kernel(AttnParams p) {
  const int bh = blockIdx.y;
  const int bi = bh / p.h, hi = bh % p.h;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int q0 = blockIdx.x * QB + w * 16;
  const int64_t tok = 3LL * p.h * D;
  const __bf16* Qb = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok + (int64_t)hi * D;
  const __bf16* Kb = Qb + (int64_t)p.h * D;
  const __bf16* Vb = Qb + 2LL * p.h * D;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[KB][D + PAD];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[KB][D + PAD];   // row-major; V^T via tr8

  bf16x8 qf[2];
  {
    const int q = q0 + c;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[ks] = q < p.s ? ld_b128(Qb + (int64_t)q * tok + 32 * ks + 8 * g) : zero8();
  }
  f32x4v O[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) O[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  const uint32_t dkey = drop_key(p.seed, (uint32_t)bh);

  for (int kb0 = 0; kb0 < p.s; kb0 += KB) {
    __syncthreads();
    {  // cooperative K / V^T block load: thread -> (key, 16 dims)
      const int t = threadIdx.x, key = t >> 2, d0 = (t & 3) * 16;
      const int kg = kb0 + key;
      bf16x8 k0 = zero8(), k1 = zero8(), v0 = zero8(), v1 = zero8();
      if (kg < p.s) {
        k0 = ld_b128(Kb + (int64_t)kg * tok + d0);
        k1 = ld_b128(Kb + (int64_t)kg * tok + d0 + 8);
        v0 = ld_b128(Vb + (int64_t)kg * tok + d0);
        v1 = ld_b128(Vb + (int64_t)kg * tok + d0 + 8);
      }
      *reinterpret_cast<bf16x8*>(&Ks[key][d0]) = k0;
      *reinterpret_cast<bf16x8*>(&Ks[key][d0 + 8]) = k1;
      *reinterpret_cast<bf16x8*>(&Vs[key][d0]) = v0;
      *reinterpret_cast<bf16x8*>(&Vs[key][d0 + 8]) = v1;
    }
    __syncthreads();
    // S^T tiles: st[t][r] = score(key kb0 + 16t + 4g + r, query q0 + c)
    float sv[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = mfma(ld_b128(&Ks[16 * t + c][32 * ks + 8 * g]), qf[ks], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb0 + 16 * t + 4 * g + r;
        float v = acc[r] * p.scale_log2;
        if (p.mask) v += (key < p.s ? p.mask[(int64_t)bi * p.s + key] : 0.f) * LOG2E;
        sv[t][r] = key < p.s ? v : -INFINITY;
      }
    }
    float mb = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) mb = fmaxf(mb, sv[t][r]);
    mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
    const float m_new = fmaxf(m_run, mb);
    const float alpha = (m_new == -INFINITY) ? 1.f : exp2f(m_run - m_new);
    float lsum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (m_new == -INFINITY) ? 0.f : exp2f(sv[t][r] - m_new);
        sv[t][r] = e;
        lsum += e;
      }
    l_run = l_run * alpha + lsum;
    m_run = m_new;
    // rescale the O rows (query 4g+r lives in lane 4g+r's column)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int n = 0; n < 4; ++n) O[n][r] *= ar;
    }
    if (p.p_drop > 0.f) {
      const uint32_t qg = (uint32_t)(q0 + c), dk = drop_key(p.seed, bh);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const uint32_t key = (uint32_t)(kb0 + 16 * t + 4 * g + r);     // even
          const uint32_t hp = drop_pair(dk, qg, key);
          sv[t][r] = drop_keep(hp, key, p.thresh) ? sv[t][r] * inv_keep : 0.f;
          sv[t][r + 1] = drop_keep(hp, key + 1, p.thresh) ? sv[t][r + 1] * inv_keep : 0.f;
        }
    }
    // O += P V  (two 32-key chunks; k order = keys 16*t0+4g+r, 16*t1+4g+r)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int t0 = 2 * ch, t1 = 2 * ch + 1;
      float a8[8] = {sv[t0][0], sv[t0][1], sv[t0][2], sv[t0][3],
                     sv[t1][0], sv[t1][1], sv[t1][2], sv[t1][3]};
      const bf16x8 af = pack8(a8);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const bf16x8 bfr = tr8(&Vs[0][0], D + PAD, 16 * t0 + 4 * g, 16 * t1 + 4 * g, 16 * n, c);
        O[n] = mfma(af, bfr, O[n]);
      }
    }
  }
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  if (g == 0 && q0 + c < p.s)
    p.lse[(int64_t)bh * p.s + q0 + c] = m_run + log2f(l_tot);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lr = __shfl(l_tot, 4 * g + r, 64);
    const float inv = lr > 0.f ? 1.f / lr : 0.f;
    const int q = q0 + 4 * g + r;
    if (q < p.s) {
      __bf16* o = ((__bf16*)p.out) + ((int64_t)bi * p.s + q) * p.h * D + (int64_t)hi * D;
#pragma unroll
      for (int n = 0; n < 4; ++n) o[16 * n + c] = (__bf16)(O[n][r] * inv);
    }
  }
}

// s <= 128 (BERT's 128-token sequences): one 8-wave workgroup per (b, h) — wave w owns
// queries 16w .. 16w + 15 — with EVERY key staged in LDS once (fwd_kernel above stages
// K / V once per 64-query block: at s = 128 twice), a one-pass softmax over all keys (no
// running max / rescale of O), dropout hashed per key pair, and the output tile written
// back through LDS as whole 128-B rows (fwd_kernel's 2-byte column stores touched 4 rows
// per instruction).
template <int OCC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(OCC))) void fwd_short_kernel(
    AttnParams p) {
  constexpr int SK = 2 * KB;
  const int bh = blockIdx.x;
  const int bi = bh / p.h, hi = bh % p.h;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int q0 = w * 16;
  const int64_t tok = 3LL * p.h * D;
  const __bf16* Qb = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok + (int64_t)hi * D;
  const __bf16* Kb = Qb + (int64_t)p.h * D;
  const __bf16* Vb = Qb + 2LL * p.h * D;
  // Ks is reused for the output tile once every wave's scores are done.  80-element rows
  // (160 B): the score's ds_read_b128 row reads of Ks and the transposed reads of Vs are
  // conflict-free on the LDS bank rules (both were 2-way with 72-element rows)
  constexpr int FP = D + 16;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[SK][FP];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[SK][FP];   // row-major; V^T via tr8

  uint32_t kmask = ~0u;
  bf16x8 qf[2];
  {
    const int q = q0 + c;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[ks] = q < p.s ? ld_b128(Qb + (int64_t)q * tok + 32 * ks + 8 * g) : zero8();
  }
  {  // 512 threads: key t / 4, dims 16 (t % 4) .. + 15 of K and of V
    const int t = threadIdx.x, key = t >> 2, d0 = (t & 3) * 16;
    bf16x8 k0 = zero8(), k1 = zero8(), v0 = zero8(), v1 = zero8();
    if (key < p.s) {
      k0 = ld_b128(Kb + (int64_t)key * tok + d0);
      k1 = ld_b128(Kb + (int64_t)key * tok + d0 + 8);
      v0 = ld_b128(Vb + (int64_t)key * tok + d0);
      v1 = ld_b128(Vb + (int64_t)key * tok + d0 + 8);
    }
    // the dropout keep bits (data-independent: hashed while the loads are in flight):
    // bit 4t + r = keep (query q0 + c, key 16t + 4g + r)
    if (p.p_drop > 0.f) {
      const uint32_t qg = (uint32_t)(q0 + c), dk = drop_key(p.seed, (uint32_t)bh);
      kmask = 0u;
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const uint32_t kk = (uint32_t)(16 * tt + 4 * g + r);          // even
          const uint32_t hp = drop_pair(dk, qg, kk);
          kmask |= ((uint32_t)drop_keep(hp, kk, p.thresh) << (4 * tt + r)) |
                   ((uint32_t)drop_keep(hp, kk + 1, p.thresh) << (4 * tt + r + 1));
        }
    }
    *reinterpret_cast<bf16x8*>(&Ks[key][d0]) = k0;
    *reinterpret_cast<bf16x8*>(&Ks[key][d0 + 8]) = k1;
    *reinterpret_cast<bf16x8*>(&Vs[key][d0]) = v0;
    *reinterpret_cast<bf16x8*>(&Vs[key][d0 + 8]) = v1;
  }
  __syncthreads();
  // S^T tiles: sv[t][r] = UNSCALED score(key 16t + 4g + r, query q0 + c) (+ mask / scale):
  // the log2-domain scale folds into the exp's argument below (one fma per element instead
  // of a multiply and a subtract), and keys past s are masked in a separate pass that a
  // full 128-key block skips (a uniform branch) instead of a select per element — the
  // kernel is VALU-bound at 6 waves per SIMD
  const float sc = p.scale_log2;
  float sv[8][4];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
    if (16 * t < p.s) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = mfma(ld_b128(&Ks[16 * t + c][32 * ks + 8 * g]), qf[ks], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 16 * t + 4 * g + r;
      float v = acc[r];
      if (p.mask) v += (key < p.s ? p.mask[(int64_t)bi * p.s + key] : 0.f) * (LOG2E / sc);
      sv[t][r] = v;
    }
  }
  if (p.s < SK) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * t + 4 * g + r >= p.s) sv[t][r] = -INFINITY;
  }
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, sv[t][r]);
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float msc = m * sc;               // the row max in the log2 domain
  float lsum = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#if MV_ATTN_RAW_EXP
      const float e = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(fmaf(sv[t][r], sc, -msc));
#else
      const float e = (m == -INFINITY) ? 0.f : exp2f(fmaf(sv[t][r], sc, -msc));
#endif
      sv[t][r] = e;
      lsum += e;
    }
  float l_tot = lsum + __shfl_xor(lsum, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
#ifdef MV_ATTN_PROBE
  if (bh == g_probe_bh && q0 + c == g_probe_q) {
    float mx = 0.f, mn = 1e30f;
    bool bad = false;
    for (int t = 0; t < 8; ++t)
      for (int r = 0; r < 4; ++r) {
        mx = fmaxf(mx, sv[t][r]);
        mn = fminf(mn, sv[t][r]);
        bad |= !(sv[t][r] == sv[t][r]);
      }
    printf("probe bh %d q %d g %d: m %g lsum %g l_tot %g e[min %g max %g] nan %d\n", bh,
           q0 + c, g, m, lsum, l_tot, mn, mx, (int)bad);
  }
#endif
  if (g == 0 && q0 + c < p.s) p.lse[(int64_t)bh * p.s + q0 + c] = msc + log2f(l_tot);
  // dropout zeroes the dropped probabilities here; the 1 / (1 - p) of the kept ones is
  // applied to O with the softmax normalisation (16 multiplies per lane instead of 32)
  const float okeep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  if (p.p_drop > 0.f) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[t][r] = ((kmask >> (4 * t + r)) & 1u) ? sv[t][r] : 0.f;
  }
  // O = P V over 32-key chunks (k order = keys 16 t0 + 4g + r, 16 t1 + 4g + r)
  f32x4v O[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) O[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    if (32 * ch >= p.s) break;
    const int t0 = 2 * ch, t1 = 2 * ch + 1;
    float a8[8] = {sv[t0][0], sv[t0][1], sv[t0][2], sv[t0][3],
                   sv[t1][0], sv[t1][1], sv[t1][2], sv[t1][3]};
    const bf16x8 af = pack8(a8);
#pragma unroll
    for (int n = 0; n < 4; ++n)
      O[n] = mfma(af, tr8(&Vs[0][0], FP, 16 * t0 + 4 * g, 16 * t1 + 4 * g, 16 * n, c), O[n]);
  }
  __syncthreads();                      // every wave is past its reads of Ks
  // lane (g, c) holds O(query q0 + 4g + r, dim 16n + c): normalise, stage the wave's 16
  // rows in Ks, read them back as 16-B pieces (4 lanes per 128-B output row)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lr = __shfl(l_tot, 4 * g + r, 64);
    const float inv = lr > 0.f ? okeep / lr : 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) Ks[q0 + 4 * g + r][16 * n + c] = (__bf16)(O[n][r] * inv);
#ifdef MV_ATTN_PROBE
    if (bh == g_probe_bh && q0 + 4 * g + r == g_probe_q)
      printf("probe out bh %d q %d c %d: lr %g O %g %g %g %g\n", bh, q0 + 4 * g + r, c, lr,
             O[0][r], O[1][r], O[2][r], O[3][r]);
#endif
  }
  __syncthreads();
  {
    const int row = q0 + (l >> 2), d0 = (l & 3) * 16;
    if (row < p.s) {
      __bf16* o = ((__bf16*)p.out) + ((int64_t)bi * p.s + row) * p.h * D + (int64_t)hi * D + d0;
      *reinterpret_cast<bf16x8*>(o) = *reinterpret_cast<const bf16x8*>(&Ks[row][d0]);
      *reinterpret_cast<bf16x8*>(o + 8) = *reinterpret_cast<const bf16x8*>(&Ks[row][d0 + 8]);
    }
  }
}

// ---------------------------------------------------------------- backward
// delta[bh, q] = sum_d dO * O
__global__ __launch_bounds__(256) void delta_kernel(const __bf16* __restrict__ out,
                                                     const __bf16* __restrict__ dout,
                                                     float* __restrict__ delta, int b, int s,
                                                     int h) {
  // 8 lanes per (b, s, h) row, 16 B each: a wave reads 8 whole 128-B rows per load
  // (one-thread-per-row touched 64 lines per instruction and ran at ~1 TB/s)
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const int j8 = (threadIdx.x & 7) * 8;
  const int64_t rows = (int64_t)b * s * h;
  float acc = 0.f;
  if (i < rows) {
    float a[8], e[8];
    load8(out + i * D + j8, a);
    load8(dout + i * D + j8, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a[j] * e[j];
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 4, 64);
  if (i < rows && j8 == 0) {
    const int hi = (int)(i % h);
    const int64_t bs = i / h;
    const int q = (int)(bs % s), bi = (int)(bs / s);
    delta[((int64_t)bi * h + hi) * s + q] = acc;
  }
}

__global__ __launch_bounds__(256) void bwd_kernel(AttnParams p, const __bf16* __restrict__ dout,
                                                   const float* __restrict__ delta,
                                                   float* __restrict__ dq_part,
                                                   __bf16* __restrict__ dqkv) {
  const int bh = blockIdx.y;
  const int bi = bh / p.h, hi = bh % p.h;
  const int kb = blockIdx.x;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int k0 = kb * KB + w * 16;
  const int64_t tok = 3LL * p.h * D;
  const int64_t otok = (int64_t)p.h * D;
  const __bf16* Qb = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok + (int64_t)hi * D;
  const __bf16* Kb = Qb + (int64_t)p.h * D;
  const __bf16* Vb = Qb + 2LL * p.h * D;
  const __bf16* dOb = dout + (int64_t)bi * p.s * otok + (int64_t)hi * D;

  __shared__ __attribute__((aligned(16))) __bf16 Qs[QB][D + PAD];
  __shared__ __attribute__((aligned(16))) __bf16 dOs[QB][D + PAD];
  __shared__ __attribute__((aligned(16))) __bf16 dSs[QB][KB + PAD];
  __shared__ __attribute__((aligned(16))) __bf16 Ks[KB][D + PAD];     // K^T via tr8
  __shared__ float lse_s[QB], del_s[QB];

  // this wave's 16 keys as MFMA B fragments (K^T / V^T columns)
  bf16x8 kf[2], vf[2];
  {
    const int key = k0 + c;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = key < p.s ? ld_b128(Kb + (int64_t)key * tok + 32 * ks + 8 * g) : zero8();
      vf[ks] = key < p.s ? ld_b128(Vb + (int64_t)key * tok + 32 * ks + 8 * g) : zero8();
    }
  }
  {  // this block's keys, row-major, for dQ = dS K
    const int t = threadIdx.x, key = t >> 2, d0 = (t & 3) * 16;
    const int kg = kb * KB + key;
    bf16x8 a = zero8(), b2 = zero8();
    if (kg < p.s) {
      a = ld_b128(Kb + (int64_t)kg * tok + d0);
      b2 = ld_b128(Kb + (int64_t)kg * tok + d0 + 8);
    }
    *reinterpret_cast<bf16x8*>(&Ks[key][d0]) = a;
    *reinterpret_cast<bf16x8*>(&Ks[key][d0 + 8]) = b2;
  }
  f32x4v dVt[4], dKt[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    dVt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    dKt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  const uint32_t dkey = drop_key(p.seed, (uint32_t)bh);
  const int keyc = k0 + c;
  const float kbias = (p.mask && keyc < p.s) ? p.mask[(int64_t)bi * p.s + keyc] * LOG2E : 0.f;
  const int nkb = (p.s + KB - 1) / KB;

  for (int qb0 = 0; qb0 < p.s; qb0 += QB) {
    __syncthreads();
    {
      const int t = threadIdx.x, row = t >> 2, d0 = (t & 3) * 16;
      const int qg = qb0 + row;
      bf16x8 q0v = zero8(), q1v = zero8(), o0 = zero8(), o1 = zero8();
      if (qg < p.s) {
        q0v = ld_b128(Qb + (int64_t)qg * tok + d0);
        q1v = ld_b128(Qb + (int64_t)qg * tok + d0 + 8);
        o0 = ld_b128(dOb + (int64_t)qg * otok + d0);
        o1 = ld_b128(dOb + (int64_t)qg * otok + d0 + 8);
      }
      *reinterpret_cast<bf16x8*>(&Qs[row][d0]) = q0v;
      *reinterpret_cast<bf16x8*>(&Qs[row][d0 + 8]) = q1v;
      *reinterpret_cast<bf16x8*>(&dOs[row][d0]) = o0;
      *reinterpret_cast<bf16x8*>(&dOs[row][d0 + 8]) = o1;
      if (t < QB) {
        const int qq = qb0 + t;
        // a query whose keys are all masked to -inf has lse = -inf (out = 0): staged as
        // +inf like a padding query, so its P is 0 (kbias - lse would be -inf + inf = NaN)
        const float lv = qq < p.s ? p.lse[(int64_t)bh * p.s + qq] : INFINITY;
        lse_s[t] = lv == -INFINITY ? INFINITY : lv;
        del_s[t] = qq < p.s ? delta[(int64_t)bh * p.s + qq] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {         // 32-query chunks
      float zc[2][4], dsc[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qt = 2 * ch + u;
        f32x4v sacc = {0.f, 0.f, 0.f, 0.f}, pacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          sacc = mfma(ld_b128(&Qs[16 * qt + c][32 * ks + 8 * g]), kf[ks], sacc);
          pacc = mfma(ld_b128(&dOs[16 * qt + c][32 * ks + 8 * g]), vf[ks], pacc);
        }
        // sacc[r] = S(q = qb0+16qt+4g+r, key = keyc); pacc[r] = dZ(q, key)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = 16 * qt + 4 * g + r;
          float pr = 0.f;
          if (keyc < p.s) pr = exp2f(sacc[r] * p.scale_log2 + kbias - lse_s[ql]);
          float z = pr, dzd = pacc[r];
          if (p.p_drop > 0.f) {
            const bool kp = keep_elem(dkey, (uint32_t)(qb0 + ql), (uint32_t)keyc, p.thresh);
            z = kp ? pr * inv_keep : 0.f;
            dzd = kp ? dzd * inv_keep : 0.f;
          }
          const float ds = pr * (dzd - del_s[ql]);
          zc[u][r] = z;
          dsc[u][r] = ds;
          dSs[ql][w * 16 + c] = (__bf16)ds;
        }
      }
      float zb[8] = {zc[0][0], zc[0][1], zc[0][2], zc[0][3], zc[1][0], zc[1][1], zc[1][2], zc[1][3]};
      float sb[8] = {dsc[0][0], dsc[0][1], dsc[0][2], dsc[0][3],
                     dsc[1][0], dsc[1][1], dsc[1][2], dsc[1][3]};
      const bf16x8 zf = pack8(zb), sf = pack8(sb);
      const int qa = 32 * ch + 4 * g, qbb = 32 * ch + 16 + 4 * g;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        dVt[n] = mfma(tr8(&dOs[0][0], D + PAD, qa, qbb, 16 * n, c), zf, dVt[n]);
        dKt[n] = mfma(tr8(&Qs[0][0], D + PAD, qa, qbb, 16 * n, c), sf, dKt[n]);
      }
    }
    __syncthreads();
    // dQ partial for 16 queries (this wave's q tile) over this block's 64 keys
    {
      const int qt = w;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc = mfma(ld_b128(&dSs[16 * qt + c][32 * ks + 8 * g]),
                     tr8(&Ks[0][0], D + PAD, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, 16 * n, c),
                     acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = qb0 + 16 * qt + 4 * g + r;
          if (q < p.s)
            dq_part[(((int64_t)kb * p.b + bi) * p.s + q) * otok + (int64_t)hi * D + 16 * n + c] =
                acc[r];
        }
      }
    }
  }
  // dK, dV: dKt[n][r] = dK^T(d = 16n+4g+r, key = keyc)
  if (keyc < p.s) {
    const float sc = p.scale_log2 / LOG2E;   // 1/sqrt(D)
    __bf16* dk = dqkv + ((int64_t)bi * p.s + keyc) * tok + (int64_t)p.h * D + (int64_t)hi * D;
    __bf16* dv = dk + (int64_t)p.h * D;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dk[16 * n + 4 * g + r] = (__bf16)(dKt[n][r] * sc);
        dv[16 * n + 4 * g + r] = (__bf16)dVt[n][r];
      }
  }
  (void)nkb;
}

// Short sequences (s <= 128, BERT pre-training's 128): ONE workgroup of 8 waves per
// (b, h) owns all (up to 2) key blocks — waves 0-3 keys 0-63, waves 4-7 keys 64-127 —
// so dQ = dS K sums over every key inside the workgroup and is written once in bf16
// (no fp32 partials, no dq_reduce pass), delta = rowsum(dO * O) is computed in the
// query-block prologue (no delta pass), and each Q / dO block is staged once for both
// key halves.
// amdgpu_waves_per_eu(4): <= 128 VGPRs, so two workgroups (76.8 KB of LDS each) share a CU;
// at 130 VGPRs only one fit (8 waves per CU on a latency-bound load -> compute -> store
// chain per (batch, head))
// bsum (optional): per-(b, h) column sums over the s tokens of dQ, dK, dV in fp32, at
// bsum[((b * 3 + which) * h + head) * 64 + d] — the fused QKV projection's bias gradient
// is their sum over b (ops/attention.py), so the separate column-sum pass over dqkv (a
// 400 MB re-read per BERT-Large layer) disappears.  Sums of the fp32 values before the
// bf16 rounding of the stored dqkv, in a fixed order (deterministic).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void bwd_short_kernel(AttnParams p,
                                                         const __bf16* __restrict__ out,
                                                         const __bf16* __restrict__ dout,
                                                         __bf16* __restrict__ dqkv,
                                                         float* __restrict__ bsum) {
  constexpr int SK = 2 * KB;     // keys per workgroup
  const int bh = blockIdx.x;
  const int bi = bh / p.h, hi = bh % p.h;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int kh = w >> 2, wq = w & 3;
  const int k0 = kh * KB + wq * 16;
  const int64_t tok = 3LL * p.h * D;
  const int64_t otok = (int64_t)p.h * D;
  const __bf16* Qb = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok + (int64_t)hi * D;
  const __bf16* Kb = Qb + (int64_t)p.h * D;
  const __bf16* Vb = Qb + 2LL * p.h * D;
  const __bf16* dOb = dout + (int64_t)bi * p.s * otok + (int64_t)hi * D;
  const __bf16* Ob = out + (int64_t)bi * p.s * otok + (int64_t)hi * D;

  // row-major images only: the k-major operands (Q^T, dO^T, K^T) come from them through
  // transposed LDS reads (tr8), so no element-wise transposed copies are written.  Round 6:
  // Q / dO of ALL queries (and delta) are staged in one prologue with K — every load of
  // the workgroup in flight at once, one barrier — instead of one load phase per 64-query
  // block (73.7 KB of LDS: still two workgroups per CU).
  // Row strides chosen on the LDS bank rules (MI355X_MICROARCH.md §LDS; computed for every
  // access of this kernel): Qs / dOs rows of 80 elements (160 B) make both their
  // ds_read_b128 row reads (4 x 16-lane groups) and their transposed reads conflict-free,
  // where the 72-element rows were 2-way on both; Ks and dSt unpadded with a chunk XOR
  // (ks_off: transposed reads conflict-free, dSt's 8-byte stores 2-way).  74.8 KB: two
  // workgroups per CU.
  constexpr int SQ = 2 * QB;
  constexpr int QP = D + 16;
  static_assert(QB == D, "dSt shares the Ks image geometry: [SK][64] with ks_off");
  __shared__ __attribute__((aligned(16))) __bf16 Qs[SQ][QP];
  __shared__ __attribute__((aligned(16))) __bf16 dOs[SQ][QP];
  // dS of the current 64-query block TRANSPOSED, [key][query] in the Ks image layout
  // (ks_off): a lane's 4 consecutive queries of one key are one 8-byte store (was 4 two-byte
  // stores), and dQ = dS K reads its A operand with transposed reads (conflict-free)
  __shared__ __attribute__((aligned(16))) __bf16 dSt[SK * QB];
  __shared__ __attribute__((aligned(16))) __bf16 Ks[SK * D];
  __shared__ __attribute__((aligned(16))) float lse_s[SQ];
  __shared__ __attribute__((aligned(16))) float del_s[SQ];

  bf16x8 kf[2], vf[2];
  {
    const int key = k0 + c;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = key < p.s ? ld_b128(Kb + (int64_t)key * tok + 32 * ks + 8 * g) : zero8();
      vf[ks] = key < p.s ? ld_b128(Vb + (int64_t)key * tok + 32 * ks + 8 * g) : zero8();
    }
  }
  {  // 512 threads: row t / 4, dims 16 (t % 4) .. + 15 of K, Q, dO (LDS) and O (delta)
    const int t = threadIdx.x, row = t >> 2, d0 = (t & 3) * 16;
    bf16x8 ka = zero8(), kb2 = zero8(), q0v = zero8(), q1v = zero8(), o0 = zero8(), o1 = zero8();
    bf16x8 y0 = zero8(), y1 = zero8();
    float lse_v = INFINITY;
    if (row < p.s) {
      ka = ld_b128(Kb + (int64_t)row * tok + d0);
      kb2 = ld_b128(Kb + (int64_t)row * tok + d0 + 8);
      q0v = ld_b128(Qb + (int64_t)row * tok + d0);
      q1v = ld_b128(Qb + (int64_t)row * tok + d0 + 8);
      o0 = ld_b128(dOb + (int64_t)row * otok + d0);
      o1 = ld_b128(dOb + (int64_t)row * otok + d0 + 8);
      y0 = ld_b128(Ob + (int64_t)row * otok + d0);
      y1 = ld_b128(Ob + (int64_t)row * otok + d0 + 8);
    }
    if (t < SQ && t < p.s) lse_v = p.lse[(int64_t)bh * p.s + t];
    // a query whose keys are all masked to -inf has lse = -inf (out = 0): staged as +inf
    // like a padding query, so its P is 0 (kbias - lse would be -inf + inf = NaN)
    if (lse_v == -INFINITY) lse_v = INFINITY;
    *reinterpret_cast<bf16x8*>(&Ks[ks_off(row, d0)]) = ka;
    *reinterpret_cast<bf16x8*>(&Ks[ks_off(row, d0 + 8)]) = kb2;
    *reinterpret_cast<bf16x8*>(&Qs[row][d0]) = q0v;
    *reinterpret_cast<bf16x8*>(&Qs[row][d0 + 8]) = q1v;
    *reinterpret_cast<bf16x8*>(&dOs[row][d0]) = o0;
    *reinterpret_cast<bf16x8*>(&dOs[row][d0 + 8]) = o1;
    if (t < SQ) lse_s[t] = lse_v;
    // delta = rowsum(dO * O): 4 lanes x 16 dims per query
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc += (float)o0[j] * (float)y0[j] + (float)o1[j] * (float)y1[j];
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if ((t & 3) == 0) del_s[row] = acc;
  }
  f32x4v dVt[4], dKt[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    dVt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    dKt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  const uint32_t dkey = drop_key(p.seed, (uint32_t)bh);
  const float qscale = p.scale_log2 / LOG2E;   // 1/sqrt(D)
  const int keyc = k0 + c;
  const float kbias = (p.mask && keyc < p.s) ? p.mask[(int64_t)bi * p.s + keyc] * LOG2E : 0.f;
  // keys past s: P = 0 by a multiply, not a branch around the exp (a divergent branch per
  // element, each with its own LDS wait, in the compiled loop)
  const float kvalid = keyc < p.s ? 1.f : 0.f;
  // dropout keep bits of this lane's key for every query (s <= 128): bit 16 (q / 64) +
  // 4 qt + r = keep (query 64 (q / 64) + 16 qt + 4g + r, key keyc).  Keys 2j and 2j + 1
  // (lanes c, c ^ 1) share one pair hash: each lane hashes half the queries (r in {0, 1}
  // or {2, 3}) for both keys and hands its partner's bits over with one lane swap.
  uint32_t kmask = ~0u;
  if (p.p_drop > 0.f) {
    uint32_t mine = 0u, theirs = 0u;
    const int rb = (c & 1) * 2;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int r = rb + rr, bit = 16 * blk + 4 * qt + r;
          const uint32_t hp = drop_pair(dkey, (uint32_t)(64 * blk + 16 * qt + 4 * g + r),
                                        (uint32_t)keyc);
          mine |= (uint32_t)drop_keep(hp, (uint32_t)keyc, p.thresh) << bit;
          theirs |= (uint32_t)drop_keep(hp, (uint32_t)keyc ^ 1u, p.thresh) << bit;
        }
    kmask = mine | (uint32_t)__shfl_xor((int)theirs, 1, 64);
  }
  __syncthreads();

  float qsum[2] = {0.f, 0.f};               // this lane's dQ column partials (bsum)
  for (int qb0 = 0; qb0 < p.s; qb0 += QB) {
    if (qb0 > 0) __syncthreads();            // the previous block's dQ reads of dSt are done
    // the lse / delta of this lane's 16 query rows of the block (16 qt + 4 g + r): four
    // 16-byte LDS reads each, one wait, instead of a read + wait per element
    f32x4v lse4[4], del4[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      lse4[qt] = *reinterpret_cast<const f32x4v*>(&lse_s[qb0 + 16 * qt + 4 * g]);
      del4[qt] = *reinterpret_cast<const f32x4v*>(&del_s[qb0 + 16 * qt + 4 * g]);
    }
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {         // 32-query chunks
      float zc[2][4], dsc[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qt = 2 * ch + u;
        f32x4v sacc = {0.f, 0.f, 0.f, 0.f}, pacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          sacc = mfma(ld_b128(&Qs[qb0 + 16 * qt + c][32 * ks + 8 * g]), kf[ks], sacc);
          pacc = mfma(ld_b128(&dOs[qb0 + 16 * qt + c][32 * ks + 8 * g]), vf[ks], pacc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // exp2f, not the raw v_exp_f32 builtin: with the builtin in the forward's
          // softmax, the compiled kernel produced NaN rows (a few queries in one test config)
          const float pr = exp2f(sacc[r] * p.scale_log2 + kbias - lse4[qt][r]) * kvalid;
          float z = pr, dzd = pacc[r];
          if (p.p_drop > 0.f) {
            const bool kp = (kmask >> ((qb0 >> 2) + 4 * qt + r)) & 1u;
            z = kp ? pr * inv_keep : 0.f;
            dzd = kp ? dzd * inv_keep : 0.f;
          }
          const float ds = pr * (dzd - del4[qt][r]);
          zc[u][r] = z;
          dsc[u][r] = ds;
        }
        // dS^T[key keyc][queries 16 qt + 4 g .. + 3]
        *reinterpret_cast<u32x2*>(&dSt[ks_off(keyc, 16 * qt + 4 * g)]) =
            u32x2{cvt_pk_bf16(dsc[u][0], dsc[u][1]), cvt_pk_bf16(dsc[u][2], dsc[u][3])};
      }
      float zb[8] = {zc[0][0], zc[0][1], zc[0][2], zc[0][3], zc[1][0], zc[1][1], zc[1][2], zc[1][3]};
      float sb[8] = {dsc[0][0], dsc[0][1], dsc[0][2], dsc[0][3],
                     dsc[1][0], dsc[1][1], dsc[1][2], dsc[1][3]};
      const bf16x8 zf = pack8(zb), sf = pack8(sb);
      const int qa = qb0 + 32 * ch + 4 * g, qbb = qb0 + 32 * ch + 16 + 4 * g;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        dVt[n] = mfma(tr8(&dOs[0][0], QP, qa, qbb, 16 * n, c), zf, dVt[n]);
        dKt[n] = mfma(tr8(&Qs[0][0], QP, qa, qbb, 16 * n, c), sf, dKt[n]);
      }
    }
    __syncthreads();
    // dQ[64 q, 64 d] = dS[64, SK] K[SK, 64]: wave -> query tile w&3, d tiles 2(w>>2)+{0,1}
    {
      const int qt = w & 3;
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) {
        const int n = 2 * (w >> 2) + nn;
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < SK / 32; ++ks)
          acc = mfma(tr8_ks(ks_base(dSt, qt, g, c), ks), tr8_ks(ks_base(Ks, n, g, c), ks), acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = qb0 + 16 * qt + 4 * g + r;
          if (q < p.s)
            dqkv[((int64_t)bi * p.s + q) * tok + (int64_t)hi * D + 16 * n + c] =
                (__bf16)(acc[r] * qscale);
        }
        qsum[nn] += ((acc[0] + acc[1]) + (acc[2] + acc[3])) * qscale;   // rows >= s are 0
      }
    }
  }
  if (bsum) {
    __syncthreads();                         // every wave is past its dQ reads of dSt
    float* red = reinterpret_cast<float*>(&dSt[0]);      // [8 waves][3][64] floats
    // dK / dV: the wave's 16 keys are the 16 lanes c of a lane group (keys >= s hold 0)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float vk = dKt[n][r], vv = dVt[n][r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          vk += __shfl_xor(vk, m, 64);
          vv += __shfl_xor(vv, m, 64);
        }
        if (c == 0) {
          red[(w * 3 + 1) * D + 16 * n + 4 * g + r] = vk * qscale;
          red[(w * 3 + 2) * D + 16 * n + 4 * g + r] = vv;
        }
      }
    // dQ: the wave's d columns 16 (2 (w >> 2) + nn) + c, summed over its rows and lane groups
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      float v = qsum[nn];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (g == 0) red[(w * 3 + 0) * D + 16 * (2 * (w >> 2) + nn) + c] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 3 * D) {
      const int which = t / D, d = t % D;
      float sum = 0.f;
      if (which == 0) {
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) sum += red[((4 * (d >> 5) + qt) * 3) * D + d];
      } else {
#pragma unroll
        for (int ww = 0; ww < 8; ++ww) sum += red[(ww * 3 + which) * D + d];
      }
      bsum[(((int64_t)bi * 3 + which) * p.h + hi) * D + d] = sum;
    }
  }
  if (keyc < p.s) {
    __bf16* dk = dqkv + ((int64_t)bi * p.s + keyc) * tok + (int64_t)p.h * D + (int64_t)hi * D;
    __bf16* dv = dk + (int64_t)p.h * D;
    // a lane's 4 consecutive d of tile n as one 8-byte store (lanes g = 0..3 of a key then
    // cover 32 contiguous bytes), not 4 two-byte stores
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float k4[4] = {dKt[n][0] * qscale, dKt[n][1] * qscale, dKt[n][2] * qscale,
                           dKt[n][3] * qscale};
      *reinterpret_cast<u32x2*>(dk + 16 * n + 4 * g) =
          u32x2{cvt_pk_bf16(k4[0], k4[1]), cvt_pk_bf16(k4[2], k4[3])};
      *reinterpret_cast<u32x2*>(dv + 16 * n + 4 * g) =
          u32x2{cvt_pk_bf16(dVt[n][0], dVt[n][1]), cvt_pk_bf16(dVt[n][2], dVt[n][3])};
    }
  }
}

__global__ __launch_bounds__(256) void dq_reduce_kernel(const float* __restrict__ dq_part,
                                                         __bf16* __restrict__ dqkv, int nkb,
                                                         int b, int s, int h, float scale) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;   // element of [b,s,h,D]
  const int64_t n = (int64_t)b * s * h * D;
  if (i >= n) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < nkb; ++k) {
    float v[8];
    load8(dq_part + (int64_t)k * n + i, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= scale;
  const int64_t row = i / D, d = i % D;          // row = (b*s + q)*h + hi (D: power of 2)
  const uint32_t r32 = (uint32_t)row, bsq32 = r32 / (uint32_t)h;   // rows < 2^32 (bindings)
  const int64_t bsq = bsq32, hi = r32 - bsq32 * (uint32_t)h;
  store8(dqkv + bsq * 3 * h * D + hi * D + d, acc);
}

}  // namespace attn
}  // namespace mv

using namespace mv::attn;


void mv_attn_fwd(const AttnParams& p, hipStream_t st) {
  if (p.s <= 2 * KB) {
    // <= 80 VGPRs (6 waves per SIMD, three workgroups per CU): 174 us vs 188 at 82 VGPRs
    // and 181 at 64 (spills) per BERT-Large layer (profiles/r6_ab_log.md)
    hipLaunchKernelGGL(fwd_short_kernel<6>, dim3(p.b * p.h), dim3(512), 0, st, p);
    return;
  }
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h);
  hipLaunchKernelGGL(fwd_kernel, grid, dim3(256), 0, st, p);
}

void mv_attn_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                 float* dq_part, void* dqkv, hipStream_t st, float* bsum) {
  if (p.s <= 2 * KB) {   // one workgroup per (b, h): no delta / dq_reduce passes
    hipLaunchKernelGGL(bwd_short_kernel, dim3(p.b * p.h), dim3(512), 0, st, p, (const __bf16*)out,
                       (const __bf16*)dout, (__bf16*)dqkv, bsum);
    return;
  }
  const int64_t rows = (int64_t)p.b * p.s * p.h;
  static_assert(D == 64, "delta_kernel maps 8 lanes x 8 elements onto a row");
  hipLaunchKernelGGL(delta_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st,
                     (const __bf16*)out, (const __bf16*)dout, delta, p.b, p.s, p.h);
  const int nkb = (p.s + KB - 1) / KB;
  hipLaunchKernelGGL(bwd_kernel, dim3(nkb, p.b * p.h), dim3(256), 0, st, p,
                     (const __bf16*)dout, (const float*)delta, dq_part, (__bf16*)dqkv);
  const int64_t n8 = rows * D / 8;
  hipLaunchKernelGGL(dq_reduce_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st,
                     (const float*)dq_part, (__bf16*)dqkv, nkb, p.b, p.s, p.h,
                     p.scale_log2 / LOG2E);
}

namespace mv {
namespace attn {
// debug / test helper: materialise the dropout keep-mask [b, h, s(q), s(k)]
__global__ void mask_kernel(int b, int h, int s, uint32_t seed, uint32_t thresh, uint8_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)b * h * s * s;
  if (i >= n) return;
  const int k = (int)(i % s);
  const int q = (int)((i / s) % s);
  const uint32_t bh = (uint32_t)(i / ((int64_t)s * s));
  keep[i] = keep_elem(drop_key(seed, bh), (uint32_t)q, (uint32_t)k, thresh) ? 1 : 0;
}
}  // namespace attn
}  // namespace mv

void mv_attn_dropout_mask(int b, int h, int s, uint32_t seed, uint32_t thresh, uint8_t* keep,
                          hipStream_t st) {
  const int64_t n = (int64_t)b * h * s * s;
  hipLaunchKernelGGL(mv::attn::mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     b, h, s, seed, thresh, keep);
}
