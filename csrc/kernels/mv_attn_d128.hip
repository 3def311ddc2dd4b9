// Fused attention at head dim 128 (docs/ATTENTION_D128.md): qkv [b, s, 3, h, 128] bf16,
// out [b, s, h, 128] bf16, lse [b, h, s] fp32 (log2 domain), fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, for any s >= 1.  Three kernels, each <SEG, CAUSAL> in all four
// forms, with the mask contract, the ranges and the dropout hash of the d = 64 kernels
// (mv_attn_kernels.h, included for Range / keys_of / queries_of / the unions / drop_* / tr8 /
// pack8; none of its kernel templates is instantiated here).
//
//   fwd128_kernel   query-block owner.  4 waves x 16 queries, Q as 4 B fragments per wave,
//                   K / V blocks of 64 keys row-major in LDS, S^T = K Q^T (a lane owns one
//                   query column), online softmax in the exp2 domain, P from the accumulators
//                   into P V (permuted k order, V^T by the transposed LDS read), 8 O tiles.
//   dq128_kernel    query-block owner, the forward's shape.  Q and dO fragments, delta =
//                   rowsum(dO * out) in the prologue (written for dkdv128_kernel), per K / V
//                   block S^T = K Q^T and dP^T = V dO^T (lse and delta are lane scalars), dS^T
//                   in the accumulators feeds dQ += dS K with K^T by the transposed read.  dQ
//                   lives in 8 register tiles over every key block and is stored once in bf16:
//                   no fp32 partials, no reduce pass, no atomics, a fixed key-block order.
//   dkdv128_kernel  key-block owner.  K and V as 4 + 4 B fragments, Q / dO blocks of 64
//                   queries through LDS, P and dP recomputed, dV^T += dO^T Z and
//                   dK^T += Q^T dS in 8 + 8 accumulator tiles.  dS never touches LDS.
//
// GQA (docs/ATTENTION_GQA.md): the same three kernels over qkv [b, s, hq + 2 hkv, 128] (a token
// holds the hq query heads, then the hkv key heads, then the hkv value heads; p.h = hq, query
// head i reads KV head i / G, G = hq / hkv).  The query-block owners give a workgroup's 64 rows
// to HW heads x 64 / HW tokens of one KV head (HW the largest of 4, 2, 1 dividing G), so a staged
// K / V block serves HW heads; the key-block owner loops over the G heads of its KV head into
// the same accumulators and stores dK / dV once.  With GQA = false all of it is compiled out.
//
// LDS images: [64][128 + LP] bf16, LP = 16: rows of 288 B.  The LDS has 64 banks of 4 B (256 B
// per pass).  (a) The transposed read (tr8): one 32-lane half reads 8 consecutive rows
// (groups g, g + 1: rows 4g .. 4g + 7), 32 B of each; row r starts at 288 r mod 256 = 32 r, so
// the 8 rows fill the 8 distinct 32-B windows.  With LP = 8 (272-B rows, what PAD = 8 would
// give) row r starts at 16 r and neighbouring rows overlap by half: 2-way.  Unpadded 256-B
// rows put all 8 rows on one window: 8-way.  (b) The ds_read_b128 row reads (lane (g, c): row
// c, bytes 64 ks + 16 g): a pass of 16 lanes is 8 rows x the lane groups g, g + 1 — the rule
// that makes mv_attn_kernels.h's recorded findings come out (160-B rows conflict-free, 144-B
// rows 2-way) — and 288 c mod 256 = 32 c gives the 8 rows distinct 32-B windows, halved by
// g: conflict-free.  (c) The staging stores: 16 lanes write one whole 256-B row.
#include "mv_attn_kernels.h"

using namespace mv;
using namespace mv::attn;

namespace {

constexpr int HD = 128;         // head dim
constexpr int NKS = HD / 32;    // MFMA k-steps over the head dim
constexpr int NDT = HD / 16;    // 16-wide output tiles over the head dim
constexpr int LP = 16;          // row padding (elements), see above
constexpr int LS = HD + LP;     // LDS row stride (elements)

typedef __bf16 Img[LS];         // one row of a [64][LS] image

// two [64][128] blocks (rows r0 .. r0 + 63 of a and b, row strides sa / sb elements; rows
// >= s read as zero) into their images: 16 lanes per 256-B row, every load of the workgroup
// in flight before the first LDS store
__device__ __forceinline__ void stage2(Img* ia, const __bf16* a, int64_t sa, Img* ib,
                                       const __bf16* b, int64_t sb, int r0, int s) {
  bf16x8 va[4], vb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + threadIdx.x, row = r0 + (idx >> 4), ch = idx & 15;
    va[i] = row < s ? ld_b128(a + (int64_t)row * sa + 8 * ch) : zero8();
    vb[i] = row < s ? ld_b128(b + (int64_t)row * sb + 8 * ch) : zero8();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + threadIdx.x, row = idx >> 4, ch = idx & 15;
    *reinterpret_cast<bf16x8*>(&ia[row][8 * ch]) = va[i];
    *reinterpret_cast<bf16x8*>(&ib[row][8 * ch]) = vb[i];
  }
}

// the 4 fragments of row `row` of a [*, 128] matrix (zero past s): lane (g, c) holds dims
// 32 ks + 8 g .. + 7 of row c, an MFMA B operand (k = dim, column = row c)
__device__ __forceinline__ void load_frags(bf16x8 (&f)[NKS], const __bf16* base, int64_t stride,
                                           int row, int g, int s) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    f[ks] = row < s ? ld_b128(base + (int64_t)row * stride + 32 * ks + 8 * g) : zero8();
}

// acc[r] = <image row 16 t + 4 g + r, the fragments' row c> over the 128 dims
__device__ __forceinline__ f32x4v dot_tile(const Img* img, int t, int g, int c,
                                           const bf16x8 (&f)[NKS]) {
  f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) acc = mfma(ld_b128(&img[16 * t + c][32 * ks + 8 * g]), f[ks], acc);
  return acc;
}

// T[n] += A x (rows ra .. ra + 3, rb .. rb + 3 of the image, columns 16 n + c): `af` holds the
// lane's 8 accumulator-born values of those rows (the permuted k order of the P V trick)
__device__ __forceinline__ void rows_into(f32x4v (&T)[NDT], const bf16x8& af, const Img* img, int ra,
                                          int rb, int c) {
#pragma unroll
  for (int n = 0; n < NDT; ++n) T[n] = mfma(af, tr8(&img[0][0], LS, ra, rb, 16 * n, c), T[n]);
}

// heavy-first block index of a query-block owner (fwd_kernel's): counted down, rotated by (b, h)
template <bool CAUSAL>
__device__ __forceinline__ int query_block() {
  return CAUSAL ? gridDim.x - 1 - (blockIdx.x + blockIdx.y) % gridDim.x : blockIdx.x;
}

struct Heads {       // per-(b, query head) base pointers into qkv
  const __bf16 *q, *k, *v;
  int64_t tok;
};
// GQA: a token is hq query heads, hkv key heads, hkv value heads; query head hi reads KV head
// hi / G
template <bool GQA>
__device__ __forceinline__ Heads heads_of(const AttnParams& p, int hkv, int bi, int hi) {
  if constexpr (GQA) {
    const int64_t tok = (int64_t)(p.h + 2 * hkv) * HD;
    const __bf16* t = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok;
    const __bf16* k = t + (int64_t)(p.h + hi / (p.h / hkv)) * HD;
    return Heads{t + (int64_t)hi * HD, k, k + (int64_t)hkv * HD, tok};
  } else {
    const int64_t tok = 3LL * p.h * HD;
    const __bf16* q = ((const __bf16*)p.qkv) + (int64_t)bi * p.s * tok + (int64_t)hi * HD;
    return Heads{q, q + (int64_t)p.h * HD, q + 2LL * p.h * HD, tok};
  }
}

// The rows of a query-block owner's wave: batch row bi, query head hi, tokens q0 .. q0 + 15.
// GQA: blockIdx.y = ((b, KV head), chunk of HW heads), blockIdx.x a tile of T = 64 / HW tokens;
// wave w takes head w % HW of the chunk and the tile's tokens from 16 (w / HW).  The K / V
// images a workgroup stages belong to its one KV head.  Under CAUSAL tile x costs
// ceil((x + 1) T / 64) key blocks: counted down and rotated like the 64-token blocks.
template <bool CAUSAL, bool GQA>
__device__ __forceinline__ void wave_rows(const AttnParams& p, int hkv, int w, int& bi, int& hi,
                                          int& q0) {
  if constexpr (GQA) {
    const int G = p.h / hkv, HW = G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1, nch = G / HW;
    const int kv = blockIdx.y / nch, ch = blockIdx.y % nch;
    const int ws = __builtin_amdgcn_readfirstlane(w);
    bi = kv / hkv;
    hi = __builtin_amdgcn_readfirstlane((kv % hkv) * G + ch * HW + ws % HW);
    q0 = __builtin_amdgcn_readfirstlane(query_block<CAUSAL>() * (QB / HW) + 16 * (ws / HW));
  } else {
    bi = blockIdx.y / p.h, hi = blockIdx.y % p.h;
    q0 = query_block<CAUSAL>() * QB + w * 16;
  }
}

// the ranges of a query-block owner: qr the keys of the lane's query, wr of the wave's 16
// queries, and the 64-key blocks [beg, end) that meet the workgroup's union (block-uniform)
template <bool SEG, bool CAUSAL>
__device__ __forceinline__ void query_ranges(const AttnParams& p, int bi, int q, Range& qr, Range& wr,
                                             int& beg, int& end) {
  qr = wr = Range{0, p.s};
  beg = 0, end = p.s;
  if constexpr (SEG || CAUSAL) {
    __shared__ int rng_s[8];
    qr = keys_of<SEG, CAUSAL>(p.seg, bi, q, p.s);
    wr = wave_union(qr);
    const Range br = block_union<4>(wr, rng_s);
    beg = min(br.lo, p.s) / KB * KB, end = br.hi;
  }
}

// ---------------------------------------------------------------- forward
template <bool SEG, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256) void fwd128_kernel(AttnParams p, int hkv) {
  constexpr bool M = SEG || CAUSAL;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  int bi, hi, q0;
  wave_rows<CAUSAL, GQA>(p, hkv, w, bi, hi, q0);
  const int bh = GQA ? bi * p.h + hi : blockIdx.y;
  const Heads hd = heads_of<GQA>(p, hkv, bi, hi);
  __shared__ __attribute__((aligned(16))) __bf16 Ks[KB][LS];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[KB][LS];       // row-major; V^T via tr8

  bf16x8 qf[NKS];
  load_frags(qf, hd.q, hd.tok, q0 + c, g, p.s);
  f32x4v O[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) O[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  const uint32_t dkey = drop_key(p.seed, (uint32_t)bh);
  Range qr, wr;
  int kb_beg, kb_end;
  query_ranges<SEG, CAUSAL>(p, bi, q0 + c, qr, wr, kb_beg, kb_end);

  for (int kb0 = kb_beg; kb0 < kb_end; kb0 += KB) {
    __syncthreads();
    stage2(Ks, hd.k, hd.tok, Vs, hd.v, hd.tok, kb0, p.s);
    __syncthreads();
    if (M && !wr.meets(kb0, KB)) continue;
    // S^T tiles: sv[t][r] = score(key kb0 + 16 t + 4 g + r, query q0 + c), log2 domain.  A
    // 16-key tile outside the wave's union is all -inf without its MFMAs
    float sv[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (M && !wr.meets(kb0 + 16 * t, 16)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sv[t][r] = -INFINITY;
        continue;
      }
      const f32x4v acc = dot_tile(Ks, t, g, c, qf);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb0 + 16 * t + 4 * g + r;
        float v = acc[r] * p.scale_log2;
        if (p.mask) v += (key < p.s ? p.mask[(int64_t)bi * p.s + key] : 0.f) * LOG2E;
        sv[t][r] = (M ? qr.has(key) : key < p.s) ? v : -INFINITY;
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
    // rescale the O rows (query 4 g + r lives in lane 4 g + r's column)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int n = 0; n < NDT; ++n) O[n][r] *= ar;
    }
    if (p.p_drop > 0.f) {
      const uint32_t qg = (uint32_t)(q0 + c);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (M && !wr.meets(kb0 + 16 * t, 16)) continue;       // P = 0 already
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const uint32_t key = (uint32_t)(kb0 + 16 * t + 4 * g + r);     // even
          const uint32_t hp = drop_pair(dkey, qg, key);
          sv[t][r] = drop_keep(hp, key, p.thresh) ? sv[t][r] * inv_keep : 0.f;
          sv[t][r + 1] = drop_keep(hp, key + 1, p.thresh) ? sv[t][r + 1] * inv_keep : 0.f;
        }
      }
    }
    // O += P V over two 32-key chunks (k order = keys 16 t0 + 4 g + r, 16 t1 + 4 g + r)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      if (M && !wr.meets(kb0 + 32 * ch, 32)) continue;       // P = 0 on all 32 keys
      const int t0 = 2 * ch, t1 = 2 * ch + 1;
      float a8[8] = {sv[t0][0], sv[t0][1], sv[t0][2], sv[t0][3],
                     sv[t1][0], sv[t1][1], sv[t1][2], sv[t1][3]};
      rows_into(O, pack8(a8), Vs, 16 * t0 + 4 * g, 16 * t1 + 4 * g, c);
    }
  }
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  if (g == 0 && q0 + c < p.s) p.lse[(int64_t)bh * p.s + q0 + c] = m_run + log2f(l_tot);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lr = __shfl(l_tot, 4 * g + r, 64);
    const float inv = lr > 0.f ? 1.f / lr : 0.f;
    const int q = q0 + 4 * g + r;
    if (q < p.s) {
      __bf16* o = ((__bf16*)p.out) + ((int64_t)bi * p.s + q) * p.h * HD + (int64_t)hi * HD;
#pragma unroll
      for (int n = 0; n < NDT; ++n) o[16 * n + c] = (__bf16)(O[n][r] * inv);
    }
  }
}

// ---------------------------------------------------------------- dQ (and delta)
template <bool SEG, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256) void dq128_kernel(AttnParams p, int hkv,
                                                     const __bf16* __restrict__ out,
                                                     const __bf16* __restrict__ dout,
                                                     float* __restrict__ delta,
                                                     __bf16* __restrict__ dqkv) {
  constexpr bool M = SEG || CAUSAL;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  int bi, hi, q0;
  wave_rows<CAUSAL, GQA>(p, hkv, w, bi, hi, q0);
  const int bh = GQA ? bi * p.h + hi : blockIdx.y, qc = q0 + c;
  const Heads hd = heads_of<GQA>(p, hkv, bi, hi);
  const int64_t otok = (int64_t)p.h * HD;
  const int64_t obase = (int64_t)bi * p.s * otok + (int64_t)hi * HD;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[KB][LS];       // row-major; K^T via tr8
  __shared__ __attribute__((aligned(16))) __bf16 Vs[KB][LS];

  bf16x8 qf[NKS], dof[NKS];
  load_frags(qf, hd.q, hd.tok, qc, g, p.s);
  load_frags(dof, dout + obase, otok, qc, g, p.s);
  // delta of query qc: the lane's 32 dims (32 ks + 8 g + j), then the 4 lane groups
  float dl = 0.f;
  {
    bf16x8 of[NKS];
    load_frags(of, out + obase, otok, qc, g, p.s);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) dl += (float)dof[ks][j] * (float)of[ks][j];
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (g == 0 && qc < p.s) delta[(int64_t)bh * p.s + qc] = dl;
  }
  // a query whose keys are all masked has lse = -inf (out = 0): taken as +inf like a query
  // past s, so its P is 0 (kbias - lse would be -inf + inf = NaN)
  float ls = qc < p.s ? p.lse[(int64_t)bh * p.s + qc] : INFINITY;
  if (ls == -INFINITY) ls = INFINITY;

  f32x4v dQ[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) dQ[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  const uint32_t dkey = drop_key(p.seed, (uint32_t)bh);
  Range qr, wr;
  int kb_beg, kb_end;
  query_ranges<SEG, CAUSAL>(p, bi, qc, qr, wr, kb_beg, kb_end);

  for (int kb0 = kb_beg; kb0 < kb_end; kb0 += KB) {
    __syncthreads();
    stage2(Ks, hd.k, hd.tok, Vs, hd.v, hd.tok, kb0, p.s);
    __syncthreads();
    if (M && !wr.meets(kb0, KB)) continue;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {       // 32-key chunks
      if (M && !wr.meets(kb0 + 32 * ch, 32)) continue;       // dS = 0 on all 32 keys
      float ds[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = 2 * ch + u;
        if (M && !wr.meets(kb0 + 16 * t, 16)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[u][r] = 0.f;
          continue;
        }
        // sacc[r] = S(key kb0 + 16 t + 4 g + r, query qc), pacc[r] = dZ of the same pair
        const f32x4v sacc = dot_tile(Ks, t, g, c, qf), pacc = dot_tile(Vs, t, g, c, dof);
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const int key = kb0 + 16 * t + 4 * g + r;       // even
          const uint32_t hp = p.p_drop > 0.f ? drop_pair(dkey, (uint32_t)qc, (uint32_t)key) : 0u;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int ke = key + e;
            float pr = 0.f;
            if (M ? qr.has(ke) : ke < p.s) {
              const float kbias = p.mask ? p.mask[(int64_t)bi * p.s + ke] * LOG2E : 0.f;
              pr = exp2f(sacc[r + e] * p.scale_log2 + kbias - ls);
            }
            float dzd = pacc[r + e];
            if (p.p_drop > 0.f) dzd = drop_keep(hp, (uint32_t)ke, p.thresh) ? dzd * inv_keep : 0.f;
            ds[u][r + e] = pr * (dzd - dl);
          }
        }
      }
      float a8[8] = {ds[0][0], ds[0][1], ds[0][2], ds[0][3], ds[1][0], ds[1][1], ds[1][2], ds[1][3]};
      rows_into(dQ, pack8(a8), Ks, 32 * ch + 4 * g, 32 * ch + 16 + 4 * g, c);
    }
  }
  // dQ[n][r] = dQ(query q0 + 4 g + r, dim 16 n + c)
  const float sc = p.scale_log2 / LOG2E;       // 1 / sqrt(128)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q < p.s) {
      __bf16* o = dqkv + ((int64_t)bi * p.s + q) * hd.tok + (int64_t)hi * HD;
#pragma unroll
      for (int n = 0; n < NDT; ++n) o[16 * n + c] = (__bf16)(dQ[n][r] * sc);
    }
  }
}

// ---------------------------------------------------------------- dK, dV
// CAUSAL: key block kb runs the query blocks from its own to the end, so ascending kb is
// heavy-first as it stands; rotated by (b, h) for the XCDs like bwd_kernel's.
// GQA: blockIdx.y = (b, KV head); the G query heads of the group run one after the other, in
// ascending order, through the same images into the same accumulators (a fixed order: two runs
// are bit-identical), and dK / dV are rounded and stored once.
template <bool SEG, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256) void dkdv128_kernel(AttnParams p, int hkv,
                                                       const __bf16* __restrict__ dout,
                                                       const float* __restrict__ delta,
                                                       __bf16* __restrict__ dqkv) {
  constexpr bool M = SEG || CAUSAL;
  const int G = GQA ? p.h / hkv : 1;       // query heads per KV head
  const int bi = blockIdx.y / (GQA ? hkv : p.h);
  const int h0 = GQA ? (blockIdx.y % hkv) * G : blockIdx.y % p.h;       // the first of them
  const int kb = CAUSAL ? (blockIdx.x + blockIdx.y) % gridDim.x : blockIdx.x;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int keyc = kb * KB + w * 16 + c;
  const Heads hd = heads_of<GQA>(p, hkv, bi, h0);
  const int64_t otok = (int64_t)p.h * HD;
  // of the head in hand: the only one, or (GQA) stepped at the end of the head loop
  int bh = GQA ? bi * p.h + h0 : blockIdx.y;
  const __bf16* Qb = hd.q;
  const __bf16* dOb = dout + (int64_t)bi * p.s * otok + (int64_t)h0 * HD;
  __shared__ __attribute__((aligned(16))) __bf16 Qs[QB][LS];        // row-major; Q^T, dO^T via tr8
  __shared__ __attribute__((aligned(16))) __bf16 dOs[QB][LS];
  __shared__ float lse_s[QB], del_s[QB];

  // this wave's 16 keys as MFMA B fragments (K^T / V^T columns)
  bf16x8 kf[NKS], vf[NKS];
  load_frags(kf, hd.k, hd.tok, keyc, g, p.s);
  load_frags(vf, hd.v, hd.tok, keyc, g, p.s);
  f32x4v dVt[NDT], dKt[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) {
    dVt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    dKt[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
  const float inv_keep = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
  uint32_t dkey = drop_key(p.seed, (uint32_t)bh);
  const float kbias = (p.mask && keyc < p.s) ? p.mask[(int64_t)bi * p.s + keyc] * LOG2E : 0.f;
  // kr = the queries of this lane's key, wr = of the wave's 16 keys, br = of the block's 64
  Range kr{0, p.s}, wr{0, p.s}, br{0, p.s};
  if constexpr (M) {
    __shared__ int rng_s[8];
    kr = queries_of<SEG, CAUSAL>(p.seg, bi, keyc, p.s);
    wr = wave_union(kr);
    br = block_union<4>(wr, rng_s);
  }
  const int qb_beg = M ? min(br.lo, p.s) / QB * QB : 0, qb_end = M ? br.hi : p.s;

  // the ranges above depend on tokens only: one set for every head of the group
  int j = 0;
  do {
    for (int qb0 = qb_beg; qb0 < qb_end; qb0 += QB) {
      __syncthreads();
      stage2(Qs, Qb, hd.tok, dOs, dOb, otok, qb0, p.s);
      if (threadIdx.x < QB) {
        const int qq = qb0 + threadIdx.x;
        // lse = -inf (a query with no key) is staged as +inf, like a query past s: P = 0
        const float lv = qq < p.s ? p.lse[(int64_t)bh * p.s + qq] : INFINITY;
        lse_s[threadIdx.x] = lv == -INFINITY ? INFINITY : lv;
        del_s[threadIdx.x] = qq < p.s ? delta[(int64_t)bh * p.s + qq] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {         // 32-query chunks
        if (M && !wr.meets(qb0 + 32 * ch, 32)) continue;       // Z = dS = 0 on all 32 queries
        float zc[2][4], dsc[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int qt = 2 * ch + u;
          if (M && !wr.meets(qb0 + 16 * qt, 16)) {       // none of these queries sees the wave's keys
#pragma unroll
            for (int r = 0; r < 4; ++r) zc[u][r] = dsc[u][r] = 0.f;
            continue;
          }
          // sacc[r] = S(query qb0 + 16 qt + 4 g + r, key keyc); pacc[r] = dZ of the same pair
          const f32x4v sacc = dot_tile(Qs, qt, g, c, kf), pacc = dot_tile(dOs, qt, g, c, vf);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = 16 * qt + 4 * g + r;
            float pr = 0.f;
            if (M ? kr.has(qb0 + ql) : keyc < p.s)
              pr = exp2f(sacc[r] * p.scale_log2 + kbias - lse_s[ql]);
            float z = pr, dzd = pacc[r];
            if (p.p_drop > 0.f) {
              const bool kp = keep_elem(dkey, (uint32_t)(qb0 + ql), (uint32_t)keyc, p.thresh);
              z = kp ? pr * inv_keep : 0.f;
              dzd = kp ? dzd * inv_keep : 0.f;
            }
            zc[u][r] = z;
            dsc[u][r] = pr * (dzd - del_s[ql]);
          }
        }
        float zb[8] = {zc[0][0], zc[0][1], zc[0][2], zc[0][3], zc[1][0], zc[1][1], zc[1][2], zc[1][3]};
        float sb[8] = {dsc[0][0], dsc[0][1], dsc[0][2], dsc[0][3],
                       dsc[1][0], dsc[1][1], dsc[1][2], dsc[1][3]};
        const bf16x8 zf = pack8(zb), sf = pack8(sb);
        const int qa = 32 * ch + 4 * g, qbb = 32 * ch + 16 + 4 * g;
#pragma unroll
        for (int n = 0; n < NDT; ++n) {
          dVt[n] = mfma(tr8(&dOs[0][0], LS, qa, qbb, 16 * n, c), zf, dVt[n]);
          dKt[n] = mfma(tr8(&Qs[0][0], LS, qa, qbb, 16 * n, c), sf, dKt[n]);
        }
      }
    }
    if constexpr (GQA) {       // the next query head of the group
      dkey = drop_key(p.seed, (uint32_t)++bh);
      Qb += HD, dOb += HD;
    }
  } while (GQA && ++j < G);
  // dKt[n][r] = dK^T(dim 16 n + 4 g + r, key keyc): 4 consecutive dims, one 8-byte store
  if (keyc < p.s) {
    const float sc = p.scale_log2 / LOG2E;   // 1 / sqrt(128)
    __bf16* dk = dqkv + ((int64_t)bi * p.s + keyc) * hd.tok + (hd.k - hd.q) + (int64_t)h0 * HD;
    __bf16* dv = dk + (hd.v - hd.k);
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      *reinterpret_cast<u32x2*>(dk + 16 * n + 4 * g) =
          u32x2{cvt_pk_bf16_cc(dKt[n][0] * sc, dKt[n][1] * sc), cvt_pk_bf16_cc(dKt[n][2] * sc, dKt[n][3] * sc)};
      *reinterpret_cast<u32x2*>(dv + 16 * n + 4 * g) =
          u32x2{cvt_pk_bf16_cc(dVt[n][0], dVt[n][1]), cvt_pk_bf16_cc(dVt[n][2], dVt[n][3])};
    }
  }
}

// hkv is read by the GQA forms only.  GQA: the query-block owners launch tiles of T = 64 / HW
// tokens by (b, KV head, chunk of HW heads), the key-block owner 64-key blocks by (b, KV head)
template <bool SEG, bool CAUSAL, bool GQA>
void launch_fwd(const AttnParams& p, int hkv, hipStream_t st) {
  // CAUSAL: blockIdx.x counts the query blocks down, rotated by (b, h): heavy first
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h);
  if constexpr (GQA) {
    const int G = p.h / hkv, HW = G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1, T = QB / HW;
    grid = dim3((p.s + T - 1) / T, p.b * hkv * (G / HW));
  }
  hipLaunchKernelGGL((fwd128_kernel<SEG, CAUSAL, GQA>), grid, dim3(256), 0, st, p, hkv);
}

template <bool SEG, bool CAUSAL, bool GQA>
void launch_bwd(const AttnParams& p, int hkv, const void* out, const void* dout, float* delta,
                void* dqkv, hipStream_t st) {
  dim3 grid((p.s + QB - 1) / QB, p.b * p.h), kgrid = grid;       // QB == KB: one grid for both owners
  if constexpr (GQA) {
    const int G = p.h / hkv, HW = G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1, T = QB / HW;
    grid = dim3((p.s + T - 1) / T, p.b * hkv * (G / HW));
    kgrid = dim3((p.s + KB - 1) / KB, p.b * hkv);
  }
  hipLaunchKernelGGL((dq128_kernel<SEG, CAUSAL, GQA>), grid, dim3(256), 0, st, p, hkv,
                     (const __bf16*)out, (const __bf16*)dout, delta, (__bf16*)dqkv);
  hipLaunchKernelGGL((dkdv128_kernel<SEG, CAUSAL, GQA>), kgrid, dim3(256), 0, st, p, hkv,
                     (const __bf16*)dout, (const float*)delta, (__bf16*)dqkv);
}

template <bool GQA>
void fwd_form(const AttnParams& p, int hkv, bool causal, hipStream_t st) {
  if (p.b * p.h == 0) return;
  if (p.seg) (causal ? launch_fwd<true, true, GQA> : launch_fwd<true, false, GQA>)(p, hkv, st);
  else (causal ? launch_fwd<false, true, GQA> : launch_fwd<false, false, GQA>)(p, hkv, st);
}

template <bool GQA>
void bwd_form(const AttnParams& p, int hkv, bool causal, const void* out, const void* dout,
              float* delta, void* dqkv, hipStream_t st) {
  if (p.b * p.h == 0) return;
  if (p.seg)
    (causal ? launch_bwd<true, true, GQA> : launch_bwd<true, false, GQA>)(p, hkv, out, dout, delta, dqkv, st);
  else
    (causal ? launch_bwd<false, true, GQA> : launch_bwd<false, false, GQA>)(p, hkv, out, dout, delta, dqkv, st);
}

}  // namespace

void mv_attn_d128_fwd(const AttnParams& p, bool causal, hipStream_t st) {
  fwd_form<false>(p, p.h, causal, st);
}

void mv_attn_d128_bwd(const AttnParams& p, bool causal, const void* out, const void* dout,
                      float* delta, void* dqkv, hipStream_t st) {
  bwd_form<false>(p, p.h, causal, out, dout, delta, dqkv, st);
}

void mv_attn_gqa_fwd(const AttnParams& p, int hkv, bool causal, hipStream_t st) {
  fwd_form<true>(p, hkv, causal, st);
}

void mv_attn_gqa_bwd(const AttnParams& p, int hkv, bool causal, const void* out, const void* dout,
                     float* delta, void* dqkv, hipStream_t st) {
  bwd_form<true>(p, hkv, causal, out, dout, delta, dqkv, st);
}
