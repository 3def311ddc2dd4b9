// One-token attention against a KV cache at head dim 128 (docs/ATTENTION_DECODE.md):
// q [b, hq, 128] bf16, kv_cache [b, S_max, 2 hkv, 128] bf16 (a token's hkv key heads, then its
// hkv value heads: the tail of the grouped qkv row), lens [b] int32 -> out [b, hq, 128] bf16,
// lse [b, hq] fp32 (log2 domain of the scaled scores).  Batch row i attends keys [0, lens[i]).
// mv_attn_kernels.h is included for mfma / tr8 / pack8 / ld_b128 / zero8; none of its kernel
// templates is instantiated here.
//
//   decode128_kernel          grid (splits, b hkv).  The work is bound by streaming K and V once
//                             and there is one query row, so the parallelism is along the keys: a
//                             workgroup owns one (batch row, KV head) and one contiguous range of
//                             the 64-key blocks of [0, lens[i]), and serves all G = hq / hkv query
//                             heads of its KV head as the 16 columns of S^T = K Q^T (columns >= G
//                             are zero; Q is 4 B fragments per wave for the whole kernel).  Each
//                             of the 4 waves takes every 4th block of the range and keeps its own
//                             online-softmax state (m, l per head column, 8 O tiles, exp2 domain)
//                             and its own V image: the key loop has no workgroup barrier.
//                             K has no reuse: lane (g, c) loads dims 32 ks + 8 g .. + 7 of key
//                             16 t + c straight into the MFMA A fragment (t, ks), 16 loads of 16 B
//                             per block.  V needs the keys as the MFMA k dimension: 16 loads of
//                             16 B per lane (16 lanes per 256-B row) go through registers into a
//                             [64][128 + 16] image (288-B rows, the bank reasons of
//                             mv_attn_d128.hip's header) and come back by the transposed read.
//                             The loads of a wave's NEXT block, 16 K + 16 V = 32 of 16 B per lane,
//                             are issued before the current block's MFMAs; the V registers are
//                             stored to the image after the block's P V.
//                             The 4 waves' states are merged through LDS once, in wave order, and
//                             one fp32 partial (m, l, o[128]) per head goes to scratch
//                             [b, hq, splits, 130].  A split with no block writes (-inf, 0, 0).
//   decode128_combine_kernel  merges the partials of a (batch row, head) in ascending split order,
//                             normalises, stores out in bf16 (one rounding) and lse.
//
// No cache row at or past lens[i] (clamped to [0, S_max]) is ever read: a lane whose key is past
// the end loads the row's last attended key instead (load_k), its V row enters the image as
// zeros and its score is -inf before the max.  No atomics: two runs with the same splits are
// bit-identical.
#include <algorithm>

#include "mv_attn_kernels.h"

using namespace mv;
using namespace mv::attn;

namespace {

constexpr int HD = 128;         // head dim
constexpr int NKS = HD / 32;    // MFMA k-steps over the head dim
constexpr int NDT = HD / 16;    // 16-wide output tiles over the head dim
constexpr int LS = HD + 16;     // image row stride (elements): 288-B rows
constexpr int NW = 4;           // waves per workgroup
constexpr int NKT = KB / 16;    // 16-key tiles per block
constexpr int NVL = KB / 4;     // V loads per lane and block (a wave covers 4 rows per load)
constexpr int PW = HD + 2;      // floats per partial: m, l, o[128]
constexpr int MS = HD + 4;      // row stride (floats) of the merge buffer

typedef __bf16 Img[LS];         // one row of a wave's [64][LS] V image

// Keys kb0 .. kb0 + 63 of one KV head as the 16 MFMA A fragments of S^T = K Q^T.  The loads are
// unconditional, so that they stay in flight over the MFMAs that follow (a load under a lane
// predicate is waited for where the predicate ends): a row >= lim (lim >= 1) reads row lim - 1
// instead, a key the row does attend.  Its score is replaced by -inf, whatever it is.
__device__ __forceinline__ void load_k(bf16x8 (&kf)[NKT][NKS], const __bf16* kb, int64_t tok,
                                       int kb0, int lim, int g, int c) {
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const __bf16* row = kb + (int64_t)min(kb0 + 16 * t + c, lim - 1) * tok + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) kf[t][ks] = ld_b128(row + 32 * ks);
  }
}

// the same keys' V rows, 16 lanes per 256-B row (load i: row 4 i + g, chunk c), clamped alike
__device__ __forceinline__ void load_v(bf16x8 (&vr)[NVL], const __bf16* vb, int64_t tok, int kb0,
                                       int lim, int g, int c) {
#pragma unroll
  for (int i = 0; i < NVL; ++i)
    vr[i] = ld_b128(vb + (int64_t)min(kb0 + 4 * i + g, lim - 1) * tok + 8 * c);
}

// into the wave's image; the rows >= lim of a partial block as zeros (P = 0 there: 0 x 0)
__device__ __forceinline__ void store_v(Img* img, bf16x8 (&vr)[NVL], int kb0, int lim, int g,
                                        int c) {
  if (kb0 + KB > lim) {       // wave-uniform
#pragma unroll
    for (int i = 0; i < NVL; ++i) vr[i] = kb0 + 4 * i + g < lim ? vr[i] : zero8();
  }
#pragma unroll
  for (int i = 0; i < NVL; ++i) *reinterpret_cast<bf16x8*>(&img[4 * i + g][8 * c]) = vr[i];
}

// orders a wave's own LDS writes and reads (the image is private to the wave: no s_barrier)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One 64-key block of a wave: S^T from the K fragments, the online softmax, O += P V from the image.
__device__ __forceinline__ void block_step(const bf16x8 (&kf)[NKT][NKS], const bf16x8 (&qf)[NKS],
                                           const Img* img, int kb0, int lim, float scale_log2,
                                           int g, int c, f32x4v (&O)[NDT], float& m_run,
                                           float& l_run) {
  // sv[t][r] = score(key kb0 + 16 t + 4 g + r, head c), log2 domain
  float sv[NKT][4];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) acc = mfma(kf[t][ks], qf[ks], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      sv[t][r] = kb0 + 16 * t + 4 * g + r < lim ? acc[r] * scale_log2 : -INFINITY;
  }
  float mb = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) mb = fmaxf(mb, sv[t][r]);
  mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
  mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
  const float m_new = fmaxf(m_run, mb);
  const float alpha = (m_new == -INFINITY) ? 1.f : exp2f(m_run - m_new);
  float lsum = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = (m_new == -INFINITY) ? 0.f : exp2f(sv[t][r] - m_new);
      sv[t][r] = e;
      lsum += e;
    }
  l_run = l_run * alpha + lsum;
  m_run = m_new;
  // rescale the O rows (head 4 g + r lives in lane 4 g + r's column)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
    for (int n = 0; n < NDT; ++n) O[n][r] *= ar;
  }
  // O += P V over two 32-key chunks (k order = keys 16 t0 + 4 g + r, 16 t1 + 4 g + r)
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const int t0 = 2 * ch, t1 = 2 * ch + 1;
    float a8[8] = {sv[t0][0], sv[t0][1], sv[t0][2], sv[t0][3],
                   sv[t1][0], sv[t1][1], sv[t1][2], sv[t1][3]};
    const bf16x8 af = pack8(a8);
#pragma unroll
    for (int n = 0; n < NDT; ++n)
      O[n] = mfma(af, tr8(&img[0][0], LS, 16 * t0 + 4 * g, 16 * t1 + 4 * g, 16 * n, c), O[n]);
  }
}

struct DecodeArgs {
  const __bf16* q;
  const __bf16* kv;
  const int* lens;
  float* part;
  int hq, hkv, s_max;
  float scale_log2;
};

__global__ __launch_bounds__(256) void decode128_kernel(DecodeArgs p) {
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const int G = p.hq / p.hkv, bi = blockIdx.y / p.hkv, kvh = blockIdx.y % p.hkv;
  const int splits = gridDim.x, sp = blockIdx.x;
  // the workgroup's blocks [b_beg, b_end) of the row's ceil(len / 64); wave w takes b_beg + w,
  // b_beg + w + 4, ...; lim ends both the row and the range
  const int len = min(max(p.lens[bi], 0), p.s_max);
  const int nblk = (len + KB - 1) / KB, per = (nblk + splits - 1) / splits;
  const int b_beg = sp * per, b_end = min(b_beg + per, nblk);
  const int lim = b_beg < b_end ? min(len, b_end * KB) : 0;
  const int64_t tok = 2LL * p.hkv * HD;
  const __bf16* kb = p.kv + (int64_t)bi * p.s_max * tok + (int64_t)kvh * HD;
  const __bf16* vb = kb + (int64_t)p.hkv * HD;
  __shared__ __attribute__((aligned(16))) __bf16 Vs[NW][KB][LS];       // row-major; V^T via tr8
  Img* img = Vs[w];

  // head kvh G + c as MFMA B fragments (k = dim, column = head); columns >= G are zero
  bf16x8 qf[NKS];
  {
    const __bf16* qb = p.q + ((int64_t)bi * p.hq + (int64_t)kvh * G + c) * HD;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = c < G ? ld_b128(qb + 32 * ks + 8 * g) : zero8();
  }
  f32x4v O[NDT];       // O[n][r] = O(head 4 g + r, dim 16 n + c)
#pragma unroll
  for (int n = 0; n < NDT; ++n) O[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  constexpr int STEP = NW * KB;
  int kb0 = (b_beg + w) * KB;
  if (kb0 < lim) {
    bf16x8 kf[NKT][NKS], vr[NVL];
    load_k(kf, kb, tok, kb0, lim, g, c);
    load_v(vr, vb, tok, kb0, lim, g, c);
    store_v(img, vr, kb0, lim, g, c);
    for (; kb0 + STEP < lim; kb0 += STEP) {
      // the wave's next block: 32 loads of 16 B per lane in flight over this block's MFMAs
      bf16x8 kn[NKT][NKS];
      load_k(kn, kb, tok, kb0 + STEP, lim, g, c);
      load_v(vr, vb, tok, kb0 + STEP, lim, g, c);
      __builtin_amdgcn_sched_barrier(0);       // all 32 issued ahead of the first MFMA
      wave_sync();
      block_step(kf, qf, img, kb0, lim, p.scale_log2, g, c, O, m_run, l_run);
      wave_sync();
      store_v(img, vr, kb0 + STEP, lim, g, c);
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) kf[t][ks] = kn[t][ks];
    }
    wave_sync();
    block_step(kf, qf, img, kb0, lim, p.scale_log2, g, c, O, m_run, l_run);
  }
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);

  // merge the 4 waves in wave order: their states go to LDS over the images
  __syncthreads();
  float* mo = reinterpret_cast<float*>(&Vs[0][0][0]);       // [NW][16][MS]
  float* mm = mo + NW * 16 * MS;                            // [NW][16]
  float* ml = mm + NW * 16;                                 // [NW][16]
  static_assert((NW * 16 * MS + 2 * NW * 16) * sizeof(float) <= sizeof(Vs), "merge buffer");
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int n = 0; n < NDT; ++n) mo[(w * 16 + 4 * g + r) * MS + 16 * n + c] = O[n][r];
  if (g == 0) {
    mm[w * 16 + c] = m_run;
    ml[w * 16 + c] = l_tot;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < G * HD; e += 256) {
    const int h = e >> 7, d = e & (HD - 1);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; ++i) m = fmaxf(m, mm[i * 16 + h]);
    float lt = 0.f, o = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const float sc = (m == -INFINITY) ? 0.f : exp2f(mm[i * 16 + h] - m);
      lt += ml[i * 16 + h] * sc;
      o += mo[(i * 16 + h) * MS + d] * sc;
    }
    float* pp = p.part + (((int64_t)bi * p.hq + (int64_t)kvh * G + h) * splits + sp) * PW;
    pp[2 + d] = o;
    if (d == 0) {
      pp[0] = m;
      pp[1] = lt;
    }
  }
}

// grid b hq, 128 threads: thread d owns dim d of one (batch row, head)
__global__ __launch_bounds__(128) void decode128_combine_kernel(const float* __restrict__ part,
                                                                 int splits,
                                                                 __bf16* __restrict__ out,
                                                                 float* __restrict__ lse) {
  const int d = threadIdx.x;
  const float* pp = part + (int64_t)blockIdx.x * splits * PW;
  float m = -INFINITY;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, pp[s * PW]);
  float lt = 0.f, o = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float sc = (m == -INFINITY) ? 0.f : exp2f(pp[s * PW] - m);
    lt += pp[s * PW + 1] * sc;
    o += pp[s * PW + 2 + d] * sc;
  }
  // no key at all (lens == 0): out = 0, lse = -inf, the dead-query contract
  out[(int64_t)blockIdx.x * HD + d] = (__bf16)(lt > 0.f ? o / lt : 0.f);
  if (d == 0) lse[blockIdx.x] = lt > 0.f ? m + log2f(lt) : -INFINITY;
}

}  // namespace

// A function of b hkv and S_max only (lens stay on the device: no host sync).  Aim at
// kDecodeWgPerCu workgroups on each of 256 CUs (the kernel's registers and LDS admit one at a
// time), with at least kDecodeMinBlocks 64-key blocks, one per wave, in a split of a full cache,
// and never more than kDecodeMaxChosen splits: past that the partials and the combine cost more
// than the shorter ranges save.  The constants come from the sweep in docs/ATTENTION_DECODE.md.
constexpr int kDecodeWgPerCu = 1;
constexpr int kDecodeMinBlocks = 4;
constexpr int kDecodeMaxChosen = 32;
static_assert(kDecodeMaxChosen <= MV_ATTN_DECODE_MAX_SPLITS, "the chosen count is a legal one");

int mv_attn_decode_splits(int b_hkv, int s_max) {
  if (b_hkv <= 0) return 1;
  const int want = (256 * kDecodeWgPerCu + b_hkv - 1) / b_hkv;
  const int cap = ((s_max + KB - 1) / KB) / kDecodeMinBlocks;
  return std::max(1, std::min(std::min(want, cap), kDecodeMaxChosen));
}

void mv_attn_decode(const AttnDecodeParams& p, hipStream_t st) {
  if (p.b == 0 || p.hq == 0) return;
  DecodeArgs a{(const __bf16*)p.q, (const __bf16*)p.kv, p.lens, p.part,
               p.hq, p.hkv, p.s_max, p.scale_log2};
  hipLaunchKernelGGL(decode128_kernel, dim3(p.splits, p.b * p.hkv), dim3(256), 0, st, a);
  hipLaunchKernelGGL(decode128_combine_kernel, dim3(p.b * p.hq), dim3(128), 0, st,
                     (const float*)p.part, p.splits, (__bf16*)p.out, p.lse);
}
