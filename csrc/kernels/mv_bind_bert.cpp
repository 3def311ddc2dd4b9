// mivod._mvk bindings: fused attention, embeddings, bias-GELU, cross entropy, LayerNorm
// (mv_attn.h, mv_bert.h; gemm_gelu_bwd also runs mv_gemm.h's 256 x 256 kernel)
#include "mv_checks.h"
#include "mv_attn.h"
#include "mv_bert.h"
#include "mv_gemm.h"

namespace {
using namespace mvc;

// contiguous bf16 tensor of exactly M * N elements
void check_mn(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
              int64_t M, int64_t N) {
  check_nd(fn, what, t, like, -1);
  TORCH_CHECK(t.numel() == M * N, fn, ": ", what, " must hold ", M * N, " elements, not ",
              t.numel());
}

// dropout threshold on a 16-bit uniform (mv_attn.hip drop_keep, mv_bert.hip keep8)
uint32_t drop_thresh(const char* fn, double p) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, fn, ": dropout must be in [0, 1)");
  return (uint32_t)std::min(65535.0, std::floor(p * 65536.0 + 0.5));
}

// ---------------------------------------------------------------------------
// Fused MFMA attention (head dim 64)
// ---------------------------------------------------------------------------
AttnParams attn_params(const char* fn, const at::Tensor& qkv, const OptTensor& mask, double p_drop,
                       int64_t seed) {
  check_nd(fn, "qkv", qkv, qkv, 5);
  TORCH_CHECK(qkv.size(2) == 3 && qkv.size(4) == 64, fn, ": qkv must be [b, s, 3, h, 64]");
  AttnParams p{};
  p.qkv = qkv.data_ptr();
  p.b = (int)qkv.size(0);
  p.s = (int)qkv.size(1);
  p.h = (int)qkv.size(3);
  p.scale_log2 = (float)(1.4426950408889634 / 8.0);
  p.mask = vec_ptr_opt(fn, "mask", mask, qkv, (int64_t)p.b * p.s);
  p.thresh = drop_thresh(fn, p_drop);
  p.p_drop = (float)p_drop;
  p.seed = (uint32_t)seed;
  TORCH_CHECK(p.s <= 65536, fn, ": sequence length must be <= 65536 (dropout counter)");
  return p;
}

std::vector<at::Tensor> attn_fwd(at::Tensor qkv, c10::optional<at::Tensor> mask, double p_drop,
                                 int64_t seed) {
  AttnParams p = attn_params("attn_fwd", qkv, mask, p_drop, seed);
  c10::DeviceGuard guard(qkv.device());
  at::Tensor out = at::empty({p.b, p.s, p.h, 64}, qkv.options());
  at::Tensor lse = at::empty({p.b, p.h, p.s}, qkv.options().dtype(at::kFloat));
  p.out = out.data_ptr();
  p.lse = lse.data_ptr<float>();
  mv_attn_fwd(p, cur_stream());
  return {out, lse};
}

// {dqkv} or (want_bsum, s <= 128) {dqkv, bsum [b, 3 h 64] fp32: the per-(b, h) column sums}
std::vector<at::Tensor> attn_bwd(const char* fn, const at::Tensor& qkv, const at::Tensor& out,
                                 const at::Tensor& dout, const at::Tensor& lse,
                                 const OptTensor& mask, double p_drop, int64_t seed,
                                 bool want_bsum) {
  AttnParams p = attn_params(fn, qkv, mask, p_drop, seed);
  const int64_t bsh = (int64_t)p.b * p.s * p.h;
  check_mn(fn, "out", out, qkv, bsh, 64);
  check_mn(fn, "dout", dout, qkv, bsh, 64);
  p.lse = vec_ptr(fn, "lse", lse, qkv, bsh);
  TORCH_CHECK(bsh < (int64_t(1) << 32), fn, ": b*s*h must be < 2^32");
  // s <= 128 runs the single-workgroup-per-(b, h) kernel: no delta / dQ partials
  const bool short_seq = p.s <= 128;
  TORCH_CHECK(!want_bsum || short_seq, fn, ": s <= 128 only");
  c10::DeviceGuard guard(qkv.device());
  auto fo = qkv.options().dtype(at::kFloat);
  const int nkb = (p.s + 63) / 64;
  at::Tensor delta = at::empty({short_seq ? 1 : (int64_t)p.b * p.h * p.s}, fo);
  at::Tensor dq_part = at::empty({short_seq ? 1 : (int64_t)nkb * p.b * p.s * p.h * 64}, fo);
  at::Tensor dqkv = at::empty_like(qkv);
  at::Tensor bsum = want_bsum ? at::empty({p.b, 3LL * p.h * 64}, fo) : at::Tensor();
  mv_attn_bwd(p, out.data_ptr(), dout.data_ptr(), delta.data_ptr<float>(),
              dq_part.data_ptr<float>(), dqkv.data_ptr(), cur_stream(),
              want_bsum ? bsum.data_ptr<float>() : nullptr);
  if (want_bsum) return {dqkv, bsum};
  return {dqkv};
}

at::Tensor attn_dropout_mask(int64_t b, int64_t h, int64_t s, double p_drop, int64_t seed,
                             at::Device device) {
  c10::DeviceGuard guard(device);
  at::Tensor keep = at::empty({b, h, s, s}, at::TensorOptions().dtype(at::kByte).device(device));
  const uint32_t th = (uint32_t)std::min(65535.0, std::floor(p_drop * 65536.0 + 0.5));
  mv_attn_dropout_mask((int)b, (int)h, (int)s, (uint32_t)seed, th, keep.data_ptr<uint8_t>(),
                       cur_stream());
  return keep;
}

// ---------------------------------------------------------------------------
// Embeddings
// ---------------------------------------------------------------------------
// embedding weight gradient: ids [T] int64, dy [T, H] bf16 -> dw [V, H] bf16 (zero rows for
// ids not in the batch); deterministic (mv_bert.hip emb_bwd_kernel)
at::Tensor embedding_bwd(at::Tensor ids, at::Tensor dy, int64_t V) {
  check_on("embedding_bwd", "ids", ids, dy, at::kLong);
  check_nd("embedding_bwd", "dy", dy, dy, 2);
  TORCH_CHECK(dy.size(0) == ids.numel() && dy.size(1) % 8 == 0,
              "embedding_bwd: dy must be [T, H] with H % 8 == 0, one row per id");
  c10::DeviceGuard guard(dy.device());
  const int64_t T = dy.size(0), H = dy.size(1);
  at::Tensor dw = at::zeros({V, H}, dy.options());
  if (T == 0) return dw;
  auto sorted = at::sort(ids.reshape({-1}), /*stable=*/true, /*dim=*/0, /*descending=*/false);
  at::Tensor sid = std::get<0>(sorted).contiguous(), perm = std::get<1>(sorted).contiguous();
  mv_embedding_bwd(dy.data_ptr(), sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), T, (int)H,
                   dw.data_ptr(), cur_stream());
  return dw;
}

// BERT embedding sum (mv_bert.hip bert_emb_fwd_kernel): ids, tt int64 [B, s]; word [V, H],
// pos [npos >= s, H], type [ntype, H] bf16 -> (y [B, s, H] bf16, bad int32 [1]: nonzero if
// any id / type was out of range, whose rows are NaN)
std::vector<at::Tensor> bert_emb_fwd(at::Tensor ids, at::Tensor tt, at::Tensor ww, at::Tensor wp,
                                     at::Tensor wt) {
  const char* fn = "bert_emb_fwd";
  check_nd(fn, "ids", ids, ww, 2, at::kLong);
  check_nd(fn, "tt", tt, ww, 2, at::kLong);
  TORCH_CHECK(ids.sizes() == tt.sizes(), "bert_emb_fwd: ids / token types must have one shape");
  check_nd(fn, "ww", ww, ww, 2);
  check_nd(fn, "wp", wp, ww, 2);
  check_nd(fn, "wt", wt, ww, 2);
  const int64_t B = ids.size(0), s = ids.size(1), H = ww.size(1);
  TORCH_CHECK(wp.size(1) == H && wt.size(1) == H, "bert_emb_fwd: tables must be [*, H] with one H");
  TORCH_CHECK(H % 8 == 0 && s <= wp.size(0) && s > 0 && wt.size(0) > 0,
              "bert_emb_fwd: H % 8 == 0, 0 < s <= position rows, >= 1 type row");
  c10::DeviceGuard guard(ww.device());
  at::Tensor y = at::empty({B, s, H}, ww.options());
  at::Tensor bad = at::zeros({1}, ids.options().dtype(at::kInt));
  mv_bert_emb_fwd(ids.data_ptr<int64_t>(), tt.data_ptr<int64_t>(), ww.data_ptr(), wp.data_ptr(),
                  wt.data_ptr(), y.data_ptr(), bad.data_ptr<int>(), B * s, (int)s, (int)H,
                  ww.size(0), (int)wt.size(0), cur_stream());
  return {y, bad};
}

// its position / token-type gradients (two types): dy [B, s, H] bf16, tt int64 [B, s] ->
// (dw_pos [npos, H] (rows >= s zero), dw_type [2, H]), fixed order (mv_bert.hip emb_pt_*)
std::vector<at::Tensor> bert_emb_pt_bwd(at::Tensor dy, at::Tensor tt, int64_t npos) {
  check_nd("bert_emb_pt_bwd", "dy", dy, dy, 3);
  check_nd("bert_emb_pt_bwd", "tt", tt, dy, 2, at::kLong);
  const int64_t B = dy.size(0), s = dy.size(1), H = dy.size(2);
  TORCH_CHECK(H % 8 == 0 && tt.size(0) == B && tt.size(1) == s,
              "bert_emb_pt_bwd: dy [B, s, H] with H % 8 == 0, token types [B, s]");
  TORCH_CHECK(s <= npos && s * H < (int64_t)1 << 31, "bert_emb_pt_bwd: s <= npos, s H < 2^31");
  c10::DeviceGuard guard(dy.device());
  at::Tensor dwp = at::zeros({npos, H}, dy.options());
  at::Tensor dwt = at::empty({2, H}, dy.options());
  if (B == 0) return {dwp, dwt.zero_()};
  const int64_t P = mv_emb_pt_partials(B, (int)s, (int)H);
  at::Tensor part = at::empty({2 * P * s * H}, dy.options().dtype(at::kFloat));
  at::Tensor ts = at::empty({2 * s * H}, dy.options().dtype(at::kFloat));
  mv_emb_pt_bwd(dy.data_ptr(), tt.data_ptr<int64_t>(), part.data_ptr<float>(),
                ts.data_ptr<float>(), dwp.data_ptr(), dwt.data_ptr(), B, (int)s, (int)H,
                cur_stream());
  return {dwp, dwt};
}

// column sums of fp32 partial rows [P, N] -> bf16 [N] (fixed order; mv_bert.hip colsum_kernel)
at::Tensor colsum_partials(at::Tensor partial) {
  check_nd("colsum_partials", "partial", partial, partial, 2, at::kFloat);
  c10::DeviceGuard guard(partial.device());
  const int64_t P = partial.size(0), N = partial.size(1);
  at::Tensor out = at::empty({N}, partial.options().dtype(at::kBFloat16));
  if (P == 0) return out.zero_();
  mv_colsum_partials(partial.data_ptr<float>(), (int)P, (int)N, out.data_ptr(), cur_stream());
  return out;
}

// ---------------------------------------------------------------------------
// Fused transformer elementwise ops (bias+GELU, cross entropy, bias+dropout+residual+LayerNorm)
// ---------------------------------------------------------------------------
at::Tensor bias_gelu_fwd(at::Tensor x, at::Tensor b) {
  const int64_t N = b.numel(), M = N ? x.numel() / N : 0;
  check_mn("bias_gelu_fwd", "x", x, x, M, N);
  check_mn("bias_gelu_fwd", "b", b, x, 1, N);
  TORCH_CHECK(N % 8 == 0 && x.size(-1) == N,
              "bias_gelu_fwd: last dim must equal bias size (%8)");
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  if (M) mv_bias_gelu_fwd(x.data_ptr(), b.data_ptr(), y.data_ptr(), M, (int)N, cur_stream());
  return y;
}

std::vector<at::Tensor> bias_gelu_bwd(at::Tensor dy, at::Tensor x, at::Tensor b) {
  const int64_t N = b.numel(), M = N ? x.numel() / N : 0;
  check_mn("bias_gelu_bwd", "dy", dy, x, M, N);
  check_mn("bias_gelu_bwd", "x", x, x, M, N);
  check_mn("bias_gelu_bwd", "b", b, x, 1, N);
  TORCH_CHECK(N % 8 == 0 && x.size(-1) == N,
              "bias_gelu_bwd: last dim must equal bias size (%8)");
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  at::Tensor db = M ? at::empty_like(b) : at::zeros_like(b);
  if (M) {
    at::Tensor partial =
        at::empty({mv_bias_gelu_partials(M, (int)N), N}, x.options().dtype(at::kFloat));
    mv_bias_gelu_bwd(dy.data_ptr(), x.data_ptr(), b.data_ptr(), dx.data_ptr(),
                     partial.data_ptr<float>(), db.data_ptr(), M, (int)N, cur_stream());
  }
  return {dx, db};
}

// cross entropy over bf16 logits [R, V] (BERT's MLM head): -> (lse [R], loss [R]) fp32
std::vector<at::Tensor> ce_fwd(at::Tensor x, at::Tensor labels, int64_t ignore) {
  check_nd("ce_fwd", "x", x, x, 2);
  const int64_t R = x.size(0), V = x.size(1);
  TORCH_CHECK(V % 2 == 0 && V > 0 && V < (int64_t(1) << 30) && R < (int64_t(1) << 31),
              "ce_fwd: vocabulary must be even");
  const int64_t* lp = vec_ptr<int64_t>("ce_fwd", "labels", labels, x, R);
  c10::DeviceGuard guard(x.device());
  at::Tensor lse = at::empty({R}, x.options().dtype(at::kFloat));
  at::Tensor loss = at::empty({R}, x.options().dtype(at::kFloat));
  if (R) mv_ce_fwd(x.data_ptr(), lp, R, (int)V, ignore, lse.data_ptr<float>(),
                   loss.data_ptr<float>(), cur_stream());
  return {lse, loss};
}

// -> dlogits bf16 [R, V] = scale * (softmax(x) - onehot(labels)), 0 rows for ignored labels
at::Tensor ce_bwd(at::Tensor x, at::Tensor labels, at::Tensor lse, at::Tensor scale, int64_t ignore) {
  check_nd("ce_bwd", "x", x, x, 2);
  const int64_t R = x.size(0), V = x.size(1);
  TORCH_CHECK(V % 2 == 0, "ce_bwd: vocabulary must be even");
  const int64_t* lp = vec_ptr<int64_t>("ce_bwd", "labels", labels, x, R);
  const float* ep = vec_ptr("ce_bwd", "lse", lse, x, R);
  const float* sp = vec_ptr("ce_bwd", "scale", scale, x, 1);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  if (R) mv_ce_bwd(x.data_ptr(), lp, ep, sp, R, (int)V, ignore, dx.data_ptr(), cur_stream());
  return dx;
}

// bias gradient of a linear layer: column sums of dy [*, N] (bf16, N % 8 == 0) -> bf16 [N]
at::Tensor bias_grad(at::Tensor dy) {
  check_nd("bias_grad", "dy", dy, dy, -1);
  TORCH_CHECK(dy.dim() >= 1, "bias_grad: dy must have a last dimension");
  const int64_t N = dy.size(-1), M = N ? dy.numel() / N : 0;
  TORCH_CHECK(N % 2 == 0 && N > 0, "bias_grad: last dim must be a positive even number");
  c10::DeviceGuard guard(dy.device());
  // the kernels load 16-B (N % 8 == 0) or 4-B vectors per row: a view at an offset that
  // breaks that alignment is summed from an aligned copy
  const uintptr_t need = N % 8 == 0 ? 16 : 4;
  if (reinterpret_cast<uintptr_t>(dy.data_ptr()) % need) dy = dy.clone();
  at::Tensor db = M ? at::empty({N}, dy.options()) : at::zeros({N}, dy.options());
  if (M && N % 8 == 0) {
    at::Tensor partial =
        at::empty({mv_bias_gelu_partials(M, (int)N), N}, dy.options().dtype(at::kFloat));
    mv_bias_grad(dy.data_ptr(), partial.data_ptr<float>(), db.data_ptr(), M, (int)N, cur_stream());
  } else if (M) {
    at::Tensor partial =
        at::empty({mv_bias_grad2_partials(M, (int)N), N}, dy.options().dtype(at::kFloat));
    mv_bias_grad2(dy.data_ptr(), partial.data_ptr<float>(), db.data_ptr(), M, (int)N, cur_stream());
  }
  return db;
}

// BERT FFN: the down projection's data gradient with the intermediate bias-GELU's backward
// in the GEMM epilogue (mv_gemm256.hip EPI 7): dy [M, K], wt = W_down^T [N, K], pre = the
// intermediate GEMM output without bias [M, N], bias [N] -> (d_pre [M, N], dbias [N] bf16)
std::vector<at::Tensor> gemm_gelu_bwd(at::Tensor dy, at::Tensor wt, at::Tensor pre, at::Tensor bias) {
  const char* fn = "gemm_gelu_bwd";
  check_nd(fn, "dy", dy, pre, 2);
  check_nd(fn, "wt", wt, pre, 2);
  check_nd(fn, "pre", pre, pre, 2);
  check_dense(fn, "bias", bias, pre);
  const int64_t M = dy.size(0), K = dy.size(1), N = wt.size(0);
  TORCH_CHECK(wt.size(1) == K && pre.size(0) == M && pre.size(1) == N && bias.numel() == N,
              "gemm_gelu_bwd: shape mismatch");
  TORCH_CHECK(M > 0 && mv_gemm256_supported(M, (int)N, (int)K) && N <= 8192,
              "gemm_gelu_bwd: unsupported shape (N % 256, K % 64, < 4 GB operands)");
  c10::DeviceGuard guard(pre.device());
  at::Tensor bf = bias.to(at::kBFloat16);
  at::Tensor d = at::empty_like(pre);
  at::Tensor db = at::empty({N}, pre.options());
  const int64_t P = mv_gemm256_partials(M, (int)N);
  at::Tensor partial = at::empty({P, 2, N}, pre.options().dtype(at::kFloat));
  const hipStream_t st = cur_stream();
  TORCH_CHECK(mv_gemm256_gelu_bwd(dy.data_ptr(), wt.data_ptr(), pre.data_ptr(), bf.data_ptr(),
                                  d.data_ptr(), partial.data_ptr<float>(), M, (int)N, (int)K, st),
              "gemm_gelu_bwd: launch rejected");
  mv_colsum_bf16(partial.data_ptr<float>(), (int)P, (int)N, 2 * N, db.data_ptr(), st);
  return {d, db};
}

std::vector<at::Tensor> ln_fwd(at::Tensor z, c10::optional<at::Tensor> bias,
                               c10::optional<at::Tensor> res, at::Tensor gamma, at::Tensor beta,
                               double eps, double p_drop, int64_t seed, bool save_v) {
  const int64_t H = gamma.numel(), M = H ? z.numel() / H : 0;
  check_mn("ln_fwd", "z", z, z, M, H);
  TORCH_CHECK(H % 8 == 0 && H <= 4096 && z.size(-1) == H,
              "ln_fwd: hidden size must be a multiple of 8, <= 4096, and match the last dim");
  check_mn("ln_fwd", "gamma", gamma, z, 1, H);
  check_mn("ln_fwd", "beta", beta, z, 1, H);
  LnFwdParams p{};
  p.z = z.data_ptr();
  if (given(bias)) {
    check_mn("ln_fwd", "bias", *bias, z, 1, H);
    p.bias = bias->data_ptr();
  }
  if (given(res)) {
    check_mn("ln_fwd", "res", *res, z, M, H);
    p.res = res->data_ptr();
  }
  p.gamma = gamma.data_ptr();
  p.beta = beta.data_ptr();
  p.thresh = drop_thresh("ln_fwd", p_drop);
  c10::DeviceGuard guard(z.device());
  at::Tensor y = at::empty_like(z);
  at::Tensor v;
  // without dropout/bias/residual the pre-LN value is z itself
  const bool v_is_z = !p.bias && !p.res && p_drop == 0.0;
  if (save_v) v = v_is_z ? z : at::empty_like(z);
  auto fo = z.options().dtype(at::kFloat);
  at::Tensor mean = at::empty({M}, fo), rstd = at::empty({M}, fo);
  p.v = (save_v && !v_is_z) ? v.data_ptr() : nullptr;
  p.y = y.data_ptr();
  p.mean = mean.data_ptr<float>();
  p.rstd = rstd.data_ptr<float>();
  p.M = M;
  p.H = (int)H;
  p.eps = (float)eps;
  p.p_drop = (float)p_drop;
  p.seed = (uint32_t)seed;
  if (M) mv_ln_fwd(p, cur_stream());
  return {y, v, mean, rstd};
}

// -> {dv, dz (undefined when p_drop == 0: equals dv), dgamma, dbeta, dbias}
std::vector<at::Tensor> ln_bwd(at::Tensor dy, at::Tensor v, at::Tensor mean, at::Tensor rstd,
                               at::Tensor gamma, double p_drop, int64_t seed, bool need_dbias,
                               c10::optional<at::Tensor> dy2) {
  const int64_t H = gamma.numel(), M = H ? dy.numel() / H : 0;
  check_mn("ln_bwd", "dy", dy, dy, M, H);
  TORCH_CHECK(H % 8 == 0 && H <= 4096, "ln_bwd: hidden size must be a multiple of 8, <= 4096");
  if (given(dy2)) check_mn("ln_bwd", "dy2", *dy2, dy, M, H);
  check_mn("ln_bwd", "v", v, dy, M, H);
  check_mn("ln_bwd", "gamma", gamma, dy, 1, H);
  LnBwdParams p{};
  p.mean = vec_ptr("ln_bwd", "mean", mean, dy, M);
  p.rstd = vec_ptr("ln_bwd", "rstd", rstd, dy, M);
  p.thresh = drop_thresh("ln_bwd", p_drop);
  c10::DeviceGuard guard(dy.device());
  at::Tensor dv = at::empty_like(dy);
  at::Tensor dz = p_drop > 0.0 ? at::empty_like(dy) : at::Tensor();
  // every column sum is written by the finalize kernel when M > 0
  auto alloc = [&]() { return M ? at::empty_like(gamma) : at::zeros_like(gamma); };
  at::Tensor dg = alloc(), db = alloc();
  at::Tensor dbias = need_dbias ? alloc() : at::Tensor();
  if (M) {
    at::Tensor partial = at::empty({mv_ln_partials(M), 3, H}, dy.options().dtype(at::kFloat));
    p.dy = dy.data_ptr();
    p.v = v.data_ptr();
    p.gamma = gamma.data_ptr();
    p.dv = dv.data_ptr();
    p.dz = dz.defined() ? dz.data_ptr() : nullptr;
    p.partial = partial.data_ptr<float>();
    p.M = M;
    p.H = (int)H;
    p.p_drop = (float)p_drop;
    p.seed = (uint32_t)seed;
    p.dy2 = given(dy2) ? dy2->data_ptr() : nullptr;
    mv_ln_bwd(p, dg.data_ptr(), db.data_ptr(), need_dbias ? dbias.data_ptr() : nullptr,
              cur_stream());
  }
  return {dv, dz, dg, db, dbias};
}

}  // namespace

void bind_bert(pybind11::module_& m) {
  using Opt = c10::optional<at::Tensor>;
  m.def("attn_fwd", &attn_fwd, "fused MFMA attention forward -> (out [b,s,h,64], lse)");
  m.def("attn_bwd",
        [](at::Tensor qkv, at::Tensor out, at::Tensor dout, at::Tensor lse, Opt mask, double p_drop,
           int64_t seed) {
          return attn_bwd("attn_bwd", qkv, out, dout, lse, mask, p_drop, seed, false)[0];
        },
        "fused MFMA attention backward -> dqkv");
  m.def("attn_dropout_mask", &attn_dropout_mask, "dropout keep-mask of the fused attention");
  m.def("bias_gelu_fwd", &bias_gelu_fwd, "y = gelu(x + b) (erf form)");
  m.def("bias_gelu_bwd", &bias_gelu_bwd, "-> (dx, dbias) of y = gelu(x + b)");
  m.def("ce_fwd", &ce_fwd, "cross entropy over bf16 logits -> (lse, per-row loss)");
  m.def("ce_bwd", &ce_bwd, "dlogits (bf16) = scale * (softmax - onehot)");
  m.def("bias_grad", &bias_grad, "column sums of dy [*, N] (bf16, N even, fixed order) -> bf16 [N]");
  m.def("colsum_partials", &colsum_partials, "column sums of fp32 partials [P, N] -> bf16 [N]");
  m.def("embedding_bwd", &embedding_bwd, "embedding weight gradient (sorted, deterministic)");
  m.def("bert_emb_fwd", &bert_emb_fwd, "word[ids] + pos[:s] + type[tt] -> (y, bad)");
  m.def("bert_emb_pt_bwd", &bert_emb_pt_bwd, "(dy, tt, npos) -> (dw_pos, dw_type) for 2 types");
  m.def("attn_bwd_bsum",
        [](at::Tensor qkv, at::Tensor out, at::Tensor dout, at::Tensor lse, Opt mask, double p_drop,
           int64_t seed) {
          return attn_bwd("attn_bwd_bsum", qkv, out, dout, lse, mask, p_drop, seed, true);
        },
        "fused MFMA attention backward (s <= 128) -> (dqkv, per-(b, h) column sums [b, 3 h 64])");
  m.def("gemm_gelu_bwd", &gemm_gelu_bwd,
        "(dy, W^T, pre, bias) -> (d_pre, dbias): dy . W with gelu(pre + bias)'s backward fused");
  m.def("ln_fwd", &ln_fwd, "v = res + dropout(z + b); y = LN(v) -> (y, v, mean, rstd)");
  m.def("ln_bwd", &ln_bwd, "-> (dv, dz, dgamma, dbeta, dbias)");
}
