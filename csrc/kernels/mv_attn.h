// Fused MFMA attention launchers — head dim 64: mv_attn.hip, mv_attn_seg.hip,
// mv_attn_causal.hip; head dim 128: mv_attn_d128.hip, mv_attn_decode.hip (one token on a KV cache).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct AttnParams {
  const void* qkv;      // bf16 [b, s, 3, h, 64]
  void* out;            // bf16 [b, s, h, 64]
  float* lse;           // [b, h, s] log2-domain log-sum-exp of the scaled scores
  const float* mask;    // [b, s] additive key bias (natural log units) or nullptr
  int b, s, h;
  float scale_log2;     // log2(e) / sqrt(64)
  float p_drop;         // attention-probability dropout
  uint32_t seed;
  uint32_t thresh;      // drop if the element's 16-bit hash < thresh (round(p_drop 2^16))
  // packed sequences: [b, s] from mv_attn_seg_bounds, token t's run of equal segment ids as
  // lo | hi << 16 (keys / queries [lo, hi); lo == hi: padding), or nullptr: dense
  const uint32_t* seg;
};

void mv_attn_fwd(const AttnParams& p, hipStream_t st);
// bsum (s <= 128 only, else must be null): fp32 [b, 3, h, 64] per-(b, h) column sums of
// dqkv over the tokens (the fused QKV projection's bias-gradient partials)
void mv_attn_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                 float* dq_part, void* dqkv, hipStream_t st, float* bsum = nullptr);
// segment ids [b, s] (int32, or int64 with ids64) -> bounds [b, s]; s <= 65535.  One launch.
void mv_attn_seg_bounds(const void* ids, bool ids64, uint32_t* bounds, int b, int s,
                        hipStream_t st);
// the p.seg != nullptr halves of mv_attn_fwd / mv_attn_bwd (which has run delta_kernel for
// s > 128): mv_attn_seg.hip
void mv_attn_seg_fwd(const AttnParams& p, hipStream_t st);
void mv_attn_seg_bwd(const AttnParams& p, const void* out, const void* dout, const float* delta,
                     float* dq_part, void* dqkv, hipStream_t st, float* bsum);
// delta[b, h, s] = rowsum(dO * out): the first pass of every s > 128 backward (mv_attn.hip)
void mv_attn_delta(const AttnParams& p, const void* out, const void* dout, float* delta,
                   hipStream_t st);
// causal attention, key j <= query i, within the run where p.seg is given (else dense lower-
// triangular, no bounds read): mv_attn_causal.hip.  The operands of mv_attn_fwd / mv_attn_bwd.
void mv_attn_causal_fwd(const AttnParams& p, hipStream_t st);
void mv_attn_causal_bwd(const AttnParams& p, const void* out, const void* dout, float* delta,
                        float* dq_part, void* dqkv, hipStream_t st, float* bsum = nullptr);
// head dim 128 (mv_attn_d128.hip): the same AttnParams over qkv [b, s, 3, h, 128] and out
// [b, s, h, 128], scale_log2 = log2(e) / sqrt(128); p.seg and causal select the form; any
// s >= 1.  delta [b, h, s] fp32 is the backward's only scratch (no dQ partials, no bsum).
void mv_attn_d128_fwd(const AttnParams& p, bool causal, hipStream_t st);
void mv_attn_d128_bwd(const AttnParams& p, bool causal, const void* out, const void* dout,
                      float* delta, void* dqkv, hipStream_t st);
// grouped-query attention at head dim 128 (the GQA forms of mv_attn_d128.hip,
// docs/ATTENTION_GQA.md): p.qkv [b, s, p.h + 2 hkv, 128], a token's p.h query heads, then hkv
// key heads, then hkv value heads; p.h % hkv == 0 and query head i reads KV head i / (p.h /
// hkv).  out, lse, delta and the dropout hash are per query head as above; dqkv in qkv's
// layout, dK / dV summed over each group in registers and stored once.
void mv_attn_gqa_fwd(const AttnParams& p, int hkv, bool causal, hipStream_t st);
void mv_attn_gqa_bwd(const AttnParams& p, int hkv, bool causal, const void* out, const void* dout,
                     float* delta, void* dqkv, hipStream_t st);
// one-token attention against a KV cache at head dim 128 (mv_attn_decode.hip,
// docs/ATTENTION_DECODE.md): batch row i's hq query heads attend keys [0, lens[i]) of its cache,
// query head j on KV head j / (hq / hkv); hq % hkv == 0, hq / hkv <= 16, b hkv <= 65535.  lens is
// read on the device and clamped to [0, s_max]; lens[i] == 0 gives out = 0, lse = -inf.
struct AttnDecodeParams {
  const void* q;        // bf16 [b, hq, 128]
  const void* kv;       // bf16 [b, s_max, 2 hkv, 128]: a token's key heads, then its value heads
  const int* lens;      // [b]
  void* out;            // bf16 [b, hq, 128]
  float* lse;           // [b, hq], log2 domain
  float* part;          // scratch fp32 [b, hq, splits, 130]: (m, l, o[128]) per split
  int b, hq, hkv, s_max;
  int splits;           // 1 .. MV_ATTN_DECODE_MAX_SPLITS workgroups along the keys
  float scale_log2;     // log2(e) / sqrt(128)
};
constexpr int MV_ATTN_DECODE_MAX_SPLITS = 64;
// the launcher's own choice of splits, from b hkv and s_max alone (no host sync on lens)
int mv_attn_decode_splits(int b_hkv, int s_max);
void mv_attn_decode(const AttnDecodeParams& p, hipStream_t st);
void mv_attn_dropout_mask(int b, int h, int s, uint32_t seed, uint32_t thresh, uint8_t* keep,
                          hipStream_t st);
