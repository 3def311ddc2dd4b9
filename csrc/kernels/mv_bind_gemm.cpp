// mivod._mvk bindings: NT GEMMs for NHWC 1x1 convolutions with their fused BN epilogues,
// and the BN fold's small products (mv_gemm.h, mv_fold.h)
#include "mv_checks.h"
#include "mv_fold.h"
#include "mv_gemm.h"

namespace {
using namespace mvc;

// contiguous bf16 [rows, cols] matrix (a negative extent is not compared)
void check_mat(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
               int64_t rows = -1, int64_t cols = -1) {
  check_nd(fn, what, t, like, 2);
  TORCH_CHECK((rows < 0 || t.size(0) == rows) && (cols < 0 || t.size(1) == cols), fn, ": ", what,
              " must be [", rows, ", ", cols, "], not ", t.sizes());
}

int64_t gemm_partials(int64_t M, int64_t N, int64_t K) {
  return mv_gemm_partials(M, (int)N, (int)K);
}

void gemm_nt(at::Tensor a, at::Tensor b, c10::optional<at::Tensor> co,
             c10::optional<at::Tensor> shift, c10::optional<at::Tensor> partial) {
  check_mat("gemm_nt", "a", a, a);
  const int64_t M = a.size(0), K = a.size(1);
  check_mat("gemm_nt", "b", b, a, -1, K);
  const int64_t N = b.size(0);
  // c = None: statistics only (C is not written) — the recompute pass of ops.bn's fold
  const bool has_c = given(co);
  if (has_c)
    check_mat("gemm_nt", "c", *co, a, M, N);
  else
    TORCH_CHECK(partial.has_value() && mv_gemm_apply_supported((int)N, (int)K),
                "gemm_nt: C may be omitted only for a statistics pass on a streamed shape");
  TORCH_CHECK(K % 64 == 0 && N % 64 == 0 && K > 0 && N > 0 && M > 0,
              "gemm_nt: K and N must be positive multiples of 64");
  TORCH_CHECK(M * K < (int64_t(1) << 40) && M * N < (int64_t(1) << 40), "gemm_nt: too large");
  TORCH_CHECK((M + 63) / 64 * (N / 64) < (int64_t(1) << 31), "gemm_nt: grid too large");
  float* pp = nullptr;
  const float* sp = nullptr;
  if (partial.has_value()) {
    pp = vec_ptr("gemm_nt", "partial", *partial, a, gemm_partials(M, N, K) * 2 * N, true);
    if (shift.has_value()) sp = vec_ptr("gemm_nt", "shift", *shift, a, N);
  }
  c10::DeviceGuard guard(a.device());
  mv_gemm_nt(a.data_ptr(), b.data_ptr(), has_c ? co->data_ptr() : nullptr, M, (int)N, (int)K, sp,
             pp, cur_stream());
}

// the 256 x 256 kernel alone (A/B against gemm_nt's routing; plain C, no statistics)
void gemm256_nt(at::Tensor a, at::Tensor b, at::Tensor c) {
  check_mat("gemm256_nt", "a", a, a);
  const int64_t M = a.size(0), K = a.size(1);
  check_mat("gemm256_nt", "b", b, a, -1, K);
  const int64_t N = b.size(0);
  check_mat("gemm256_nt", "c", c, a, M, N);
  TORCH_CHECK(mv_gemm256_supported(M, (int)N, (int)K),
              "gemm256_nt: needs N % 256 == 0 and K % 64 == 0");
  c10::DeviceGuard guard(a.device());
  mv_gemm256_nt(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, (int)N, (int)K, nullptr, nullptr,
                cur_stream());
}

// strided 1x1 conv forward on the 256 x 256 kernel: y[Nb, Ho, Wo, N] (NHWC, returned as
// channels_last NCHW) = conv1x1(x, w, stride ds), + BN statistics partials when shift is
// given; None when the shape is not covered
c10::optional<std::vector<at::Tensor>> conv1x1_strided_stats(at::Tensor x, at::Tensor w, int64_t ds,
                                                             c10::optional<at::Tensor> shift) {
  const char* fn = "conv1x1_strided_stats";
  check_chlast(fn, "x", x, x);
  check_on(fn, "w", w, x, at::kBFloat16);  // any layout: reshaped to a contiguous [N, C] below
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 1 && w.size(3) == 1 && w.size(1) == x.size(1),
              "conv1x1_strided_stats: w must be a [N, C, 1, 1] filter");
  TORCH_CHECK(ds >= 1, "conv1x1_strided_stats: stride >= 1");
  const int64_t Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3), N = w.size(0);
  const int64_t Ho = (H - 1) / ds + 1, Wo = (W - 1) / ds + 1, M = Nb * Ho * Wo;
  const float* sp = shift.has_value() ? vec_ptr(fn, "shift", *shift, x, N) : nullptr;
  if (!mv_gemm256_supported(M, (int)N, (int)C) || (sp && N > 8192)) return c10::nullopt;
  c10::DeviceGuard guard(x.device());
  at::Tensor w2 = w.reshape({N, C}).contiguous();
  at::Tensor y = at::empty({Nb, N, Ho, Wo}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor part;
  float* pp = nullptr;
  if (sp) {
    part = at::empty({mv_gemm256_partials(M, (int)N), 2, N}, x.options().dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  if (!mv_gemm256_strided(x.data_ptr(), w2.data_ptr(), y.data_ptr(), (int)Nb, (int)H, (int)W,
                          (int)C, (int)N, (int)ds, sp, pp, cur_stream()))
    return c10::nullopt;
  std::vector<at::Tensor> out{y};
  if (pp) out.push_back(part);
  return out;
}

int64_t gemm_fold_dx_partials(int64_t M, int64_t K1, int64_t K2) {
  return mv_gemm_fold_dx_partials(M, (int)K1, (int)K2);
}

// The BN3 fold's data gradient with BN2's ReLU backward reduce: d = relu'(bn2(xb)) *
// ([a1 | a2] . b^T + badd) -> d (bf16 [M, K2]); returns the [P, 2, K2] partials
at::Tensor gemm_fold_dx(at::Tensor a1, at::Tensor a2, at::Tensor b, at::Tensor badd, at::Tensor d,
                        at::Tensor xb, at::Tensor vec) {
  const char* fn = "gemm_fold_dx";
  check_mat(fn, "a1", a1, a1);
  const int64_t M = a1.size(0), K1 = a1.size(1);
  check_mat(fn, "a2", a2, a1, M);
  const int64_t K2 = a2.size(1);
  check_mat(fn, "b", b, a1, K2, K1 + K2);
  check_mat(fn, "d", d, a1, M, K2);
  check_mat(fn, "xb", xb, a1, M, K2);
  TORCH_CHECK(M > 0 && M * (K1 + K2) < (int64_t(1) << 40), "gemm_fold_dx: empty or too large");
  const float* bp = vec_ptr(fn, "badd", badd, a1, K2);
  const float* vp = vec_ptr(fn, "vec", vec, a1, 4 * K2);
  const int64_t P = mv_gemm_fold_dx_partials(M, (int)K1, (int)K2);
  TORCH_CHECK(P > 0, "gemm_fold_dx: unsupported (K1, K2)");
  c10::DeviceGuard guard(a1.device());
  at::Tensor partial = at::empty({P, 2, K2}, a1.options().dtype(at::kFloat));
  TORCH_CHECK(mv_gemm_fold_dx(a1.data_ptr(), a2.data_ptr(), b.data_ptr(), bp, d.data_ptr(), M,
                              (int)K1, (int)K2, xb.data_ptr(), vp, vp + 2 * K2, vp + 3 * K2,
                              partial.data_ptr<float>(), cur_stream()),
              "gemm_fold_dx: launch failed");
  return partial;
}

bool gemm_dual_supported(int64_t K1, int64_t K2) { return mv_gemm_dual_supported((int)K1, (int)K2); }

// D [M, N] = [A1 | x[:, :, ::s, ::s]] . B^T + badd on the 256 x 256 pipeline with the second
// source gathered from the channels_last x [Nb, K2, H, W] (no strided copy); false when the
// shape is not covered (N % 256 or the K splits)
bool gemm_dual_bias_strided(at::Tensor a1, at::Tensor x, int64_t stride, at::Tensor b,
                            at::Tensor badd, at::Tensor d) {
  const char* fn = "gemm_dual_bias_strided";
  check_mat(fn, "a1", a1, a1);
  check_chlast(fn, "x", x, a1);
  TORCH_CHECK(stride >= 1 && stride < 65536 && x.size(2) < 65536 && x.size(3) < 65536,
              "gemm_dual_bias_strided: bad stride / size");
  const int64_t M = a1.size(0), K1 = a1.size(1), K2 = x.size(1);
  const int64_t H = x.size(2), W = x.size(3);
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  TORCH_CHECK(M == x.size(0) * Ho * Wo, "gemm_dual_bias_strided: shape mismatch");
  check_mat(fn, "b", b, a1, -1, K1 + K2);
  const int64_t N = b.size(0);
  check_mat(fn, "d", d, a1, M, N);
  const float* bp = vec_ptr(fn, "badd", badd, a1, N);
  c10::DeviceGuard guard(a1.device());
  return mv_gemm256_dual(a1.data_ptr(), x.data_ptr(), b.data_ptr(), bp, d.data_ptr(), M, (int)K1,
                         (int)K2, (int)N, nullptr, nullptr, nullptr, nullptr, nullptr,
                         cur_stream(), (int)stride, (int)H, (int)W);
}

// d = [a1 | a2] . b^T + badd (bf16 [M, K2])
void gemm_dual_bias(at::Tensor a1, at::Tensor a2, at::Tensor b, at::Tensor badd, at::Tensor d) {
  const char* fn = "gemm_dual_bias";
  check_mat(fn, "a1", a1, a1);
  const int64_t M = a1.size(0), K1 = a1.size(1);
  check_mat(fn, "a2", a2, a1, M);
  const int64_t K2 = a2.size(1);
  check_mat(fn, "b", b, a1, K2, K1 + K2);
  check_mat(fn, "d", d, a1, M, K2);
  TORCH_CHECK(M > 0 && M * (K1 + K2) < (int64_t(1) << 40), "gemm_dual_bias: empty or too large");
  const float* bp = vec_ptr(fn, "badd", badd, a1, K2);
  TORCH_CHECK(mv_gemm_dual_supported((int)K1, (int)K2), "gemm_dual_bias: unsupported (K1, K2)");
  c10::DeviceGuard guard(a1.device());
  TORCH_CHECK(mv_gemm_dual_bias(a1.data_ptr(), a2.data_ptr(), b.data_ptr(), bp, d.data_ptr(), M,
                                (int)K1, (int)K2, cur_stream()),
              "gemm_dual_bias: launch failed");
}

// [1, 2, cout] BN statistics partials of z = x W^T around shift from the Gram matrix
// gram = x^T x ([cin, cin] fp32) and xsum = colsum(x) [cin] (mv_fold.hip gram_stats_kernel)
at::Tensor gram_stats(at::Tensor w, at::Tensor gram, at::Tensor xsum,
                      c10::optional<at::Tensor> shift, int64_t m) {
  check_mat("gram_stats", "w", w, w);
  const int64_t cout = w.size(0), cin = w.size(1);
  const float* gp = vec_ptr("gram_stats", "gram", gram, w, cin * cin);
  const float* xp = vec_ptr("gram_stats", "xsum", xsum, w, cin);
  const float* sh = vec_ptr_opt("gram_stats", "shift", shift, w, cout);
  TORCH_CHECK(m > 0, "gram_stats: m must be positive");
  c10::DeviceGuard guard(w.device());
  at::Tensor part = at::empty({1, 2, cout}, gram.options());
  TORCH_CHECK(mv_gram_stats(w.data_ptr(), gp, xp, sh, m, (int)cout, (int)cin,
                            part.data_ptr<float>(), cur_stream()),
              "gram_stats: needs cout % 16 == 0 and cin <= 1024");
  return part;
}

// {co [5, cout], xsum [cin]}: the BN fold's per-channel coefficients from the consumer's
// reduce partials part [P, 2, cout], W [cout, cin] (bf16), g = dz^T x [cout, cin] (fp32),
// the BN's saved vec [4, cout] and gamma; xsum from colsum partials [P2, cin] (or zeros
// when colsum is None — the caller supplies it)
std::vector<at::Tensor> fold_coeffs(at::Tensor part, at::Tensor w, at::Tensor g, at::Tensor vec,
                                    c10::optional<at::Tensor> gamma, int64_t M,
                                    c10::optional<at::Tensor> colsum) {
  const char* fn = "fold_coeffs";
  check_nd(fn, "part", part, w, 3, at::kFloat);
  check_mat(fn, "w", w, w);
  const int64_t cout = w.size(0), cin = w.size(1);
  TORCH_CHECK(part.size(0) > 0 && part.size(1) == 2 && part.size(2) == cout,
              "fold_coeffs: part must be fp32 [P, 2, cout]");
  const float* gp = vec_ptr(fn, "g", g, w, cout * cin);
  const float* vp = vec_ptr(fn, "vec", vec, w, 4 * cout);
  const float* gm = vec_ptr_opt(fn, "gamma", gamma, w, cout);
  const float* cs = nullptr;
  int P2 = 0;
  if (given(colsum)) {
    check_nd(fn, "colsum", *colsum, w, 2, at::kFloat);
    TORCH_CHECK(colsum->size(1) == cin, "fold_coeffs: colsum must be fp32 [P2, cin]");
    cs = colsum->data_ptr<float>();
    P2 = (int)colsum->size(0);
  }
  TORCH_CHECK(M > 0, "fold_coeffs: M must be positive");
  c10::DeviceGuard guard(w.device());
  at::Tensor co = at::empty({5, cout}, part.options());
  at::Tensor xsum = cs ? at::empty({cin}, part.options()) : at::zeros({cin}, part.options());
  mv_fold_coeffs(part.data_ptr<float>(), (int)part.size(0), w.data_ptr(), gp, vp, gm, M, (int)cout,
                 (int)cin, cs, P2, co.data_ptr<float>(), xsum.data_ptr<float>(), cur_stream());
  return {co, xsum};
}

// {dW bf16 [cout, cin] (undefined if not need_w), bcat bf16 [cin, cout + cin], badd fp32 [cin]}
std::vector<at::Tensor> fold_products(at::Tensor w, at::Tensor g, c10::optional<at::Tensor> gram,
                                      at::Tensor co, at::Tensor xsum, bool need_w) {
  const char* fn = "fold_products";
  check_mat(fn, "w", w, w);
  const int64_t cout = w.size(0), cin = w.size(1);
  TORCH_CHECK(cout % 64 == 0 && cin % 64 == 0 && cout > 0 && cin > 0,
              "fold_products: channels must be positive multiples of 64 (64x64 tiles)");
  const float* gp = vec_ptr(fn, "g", g, w, cout * cin);
  const float* cp = vec_ptr(fn, "co", co, w, 5 * cout);
  const float* xp = vec_ptr(fn, "xsum", xsum, w, cin);
  const float* gr = nullptr;
  if (need_w) {
    TORCH_CHECK(given(gram), "fold_products: need_w needs the Gram matrix");
    gr = vec_ptr(fn, "gram", *gram, w, cin * cin);
  }
  c10::DeviceGuard guard(w.device());
  at::Tensor dw = need_w ? at::empty({cout, cin}, w.options()) : at::Tensor();
  at::Tensor bcat = at::empty({cin, cout + cin}, w.options());
  at::Tensor badd = at::empty({cin}, co.options());
  mv_fold_products(w.data_ptr(), gp, gr, cp, xp, (int)cout, (int)cin,
                   need_w ? dw.data_ptr() : nullptr, bcat.data_ptr(), badd.data_ptr<float>(),
                   cur_stream());
  return {dw, bcat, badd};
}

bool gemm_apply_supported(int64_t N, int64_t K) { return mv_gemm_apply_supported((int)N, (int)K); }

// {y, mask}: y = relu(bf16(a . b^T) * scale + bias + res) and its [M, N/8] bitmask (the
// GEMM recomputed with the BN+add+ReLU apply in its epilogue)
std::vector<at::Tensor> gemm_nt_apply(at::Tensor a, at::Tensor b, at::Tensor res, at::Tensor scale,
                                      at::Tensor bias, c10::optional<at::Tensor> rscale,
                                      c10::optional<at::Tensor> rbias) {
  const char* fn = "gemm_nt_apply";
  check_mat(fn, "a", a, a);
  const int64_t M = a.size(0), K = a.size(1);
  check_mat(fn, "b", b, a, -1, K);
  const int64_t N = b.size(0);
  check_mat(fn, "res", res, a, M, N);
  TORCH_CHECK(M > 0 && mv_gemm_apply_supported((int)N, (int)K),
              "gemm_nt_apply: empty or unsupported (K, N)");
  TORCH_CHECK(M * K < (int64_t(1) << 40) && M * N < (int64_t(1) << 40), "gemm_nt_apply: too large");
  const float* sp = vec_ptr(fn, "scale", scale, a, N);
  const float* bp = vec_ptr(fn, "bias", bias, a, N);
  const float* rsp = vec_ptr_opt(fn, "rscale", rscale, a, N);
  const float* rbp = vec_ptr_opt(fn, "rbias", rbias, a, N);
  TORCH_CHECK((rsp == nullptr) == (rbp == nullptr), "gemm_nt_apply: rscale and rbias go together");
  c10::DeviceGuard guard(a.device());
  at::Tensor y = at::empty({M, N}, res.options());
  at::Tensor mask = at::empty({M, N / 8}, res.options().dtype(at::kByte));
  TORCH_CHECK(mv_gemm_nt_apply(a.data_ptr(), b.data_ptr(), y.data_ptr(), M, (int)N, (int)K,
                               res.data_ptr(), sp, bp, mask.data_ptr(), cur_stream(), rsp, rbp),
              "gemm_nt_apply: launch failed");
  return {y, mask};
}

bool gemm_apply_dual_supported(int64_t N, int64_t K) {
  return mv_gemm_apply_dual_supported((int)N, (int)K);
}

// {y, mask}: relu(bf16(a . b^T) * scale + bias + bf16(bf16(a2 . b2^T) * rscale + rbias))
std::vector<at::Tensor> gemm_nt_apply_dual(at::Tensor a, at::Tensor b, at::Tensor a2,
                                           at::Tensor b2, at::Tensor scale, at::Tensor bias,
                                           at::Tensor rscale, at::Tensor rbias) {
  const char* fn = "gemm_nt_apply_dual";
  check_mat(fn, "a", a, a);
  const int64_t M = a.size(0), K = a.size(1);
  check_mat(fn, "b", b, a, -1, K);
  const int64_t N = b.size(0);
  check_mat(fn, "a2", a2, a, M, K);
  check_mat(fn, "b2", b2, a, N, K);
  TORCH_CHECK(M > 0 && M * N < (int64_t(1) << 40) && mv_gemm_apply_dual_supported((int)N, (int)K),
              "gemm_nt_apply_dual: empty, too large or unsupported (K, N)");
  const float* sp = vec_ptr(fn, "scale", scale, a, N);
  const float* bp = vec_ptr(fn, "bias", bias, a, N);
  const float* rsp = vec_ptr(fn, "rscale", rscale, a, N);
  const float* rbp = vec_ptr(fn, "rbias", rbias, a, N);
  c10::DeviceGuard guard(a.device());
  at::Tensor y = at::empty({M, N}, a.options());
  at::Tensor mask = at::empty({M, N / 8}, a.options().dtype(at::kByte));
  TORCH_CHECK(mv_gemm_nt_apply_dual(a.data_ptr(), b.data_ptr(), a2.data_ptr(), b2.data_ptr(),
                                    y.data_ptr(), M, (int)N, (int)K, sp, bp, rsp, rbp,
                                    mask.data_ptr(), cur_stream()),
              "gemm_nt_apply_dual: launch failed");
  return {y, mask};
}

int64_t gemm_bwd_partials(int64_t M, int64_t N, int64_t K, int64_t bn) {
  return mv_gemm_bwd_partials(M, (int)N, (int)K, (int)bn);
}

// Data-gradient GEMM of a 1x1 conv fused with the BN+add+ReLU (mode 3) backward
// reduce of the BN that produced the conv's input: dy = a . b^T, dz = mask ? dy + dy2
// : 0 is written to dz, returns the fp32 [P, 2, N] partials (sum dz, sum dz (x - mean)).
// x = None: only sum dz (the second partial is 0; ops.bn._Conv1x1BNFold gets it from its
// weight-gradient GEMM) and the BN input is never read.
at::Tensor gemm_nt_bn_bwd(at::Tensor a, at::Tensor b, at::Tensor dz,
                          c10::optional<at::Tensor> dy2, at::Tensor mask,
                          c10::optional<at::Tensor> xo, at::Tensor vec, int64_t bn,
                          int64_t dy2_stride, int64_t H, int64_t W) {
  const char* fn = "gemm_nt_bn_bwd";
  check_mat(fn, "a", a, a);
  const int64_t M = a.size(0), K = a.size(1);
  check_mat(fn, "b", b, a, -1, K);
  const int64_t N = b.size(0);
  TORCH_CHECK(M > 0 && M * N < (int64_t(1) << 40) && N % 64 == 0, "gemm_nt_bn_bwd: bad size");
  // dz / x: [M, N] in memory (2-D, or the NHWC activation seen as any contiguous view)
  check_nd(fn, "dz", dz, a, -1);
  TORCH_CHECK(dz.numel() == M * N, "gemm_nt_bn_bwd: dz must be [M, N]");
  const void* xp = nullptr;
  if (given(xo)) {
    check_nd(fn, "x", *xo, a, -1);
    TORCH_CHECK(xo->numel() == M * N, "gemm_nt_bn_bwd: x must be [M, N]");
    xp = xo->data_ptr();
  }
  const int64_t P = gemm_bwd_partials(M, N, K, bn);
  TORCH_CHECK(P > 0, "gemm_nt_bn_bwd: unsupported (K, N) — K must be 64, 128 or 256");
  const uint8_t* mp = vec_ptr<uint8_t>(fn, "mask", mask, a, M * (N / 8));
  const float* vp = vec_ptr(fn, "vec", vec, a, 4 * N);
  const void* d2 = nullptr;
  TORCH_CHECK(dy2_stride >= 1, "gemm_nt_bn_bwd: bad dy2 stride");
  if (given(dy2)) {
    if (dy2->dim() == 4)
      check_chlast(fn, "dy2", *dy2, a);
    else
      check_nd(fn, "dy2", *dy2, a, -1);
    TORCH_CHECK(dy2->dim() != 4 || dy2->size(1) == N, "gemm_nt_bn_bwd: dy2 must be bf16 [*, N]");
    if (dy2_stride == 1) {
      TORCH_CHECK(dy2->numel() == M * N, "gemm_nt_bn_bwd: dy2 must be [M, N]");
    } else {
      TORCH_CHECK(H > 0 && W > 0 && M % (H * W) == 0 && M < (int64_t(1) << 31),
                  "gemm_nt_bn_bwd: strided dy2 needs M = n*H*W < 2^31");
      const int64_t s = dy2_stride, hs = (H + s - 1) / s, ws = (W + s - 1) / s;
      TORCH_CHECK(dy2->dim() == 4 && dy2->size(0) == M / (H * W) && dy2->size(2) == hs &&
                      dy2->size(3) == ws,
                  "gemm_nt_bn_bwd: strided dy2 must be [n, N, ceil(H/s), ceil(W/s)]");
    }
    d2 = dy2->data_ptr();
  }
  c10::DeviceGuard guard(a.device());
  at::Tensor partial = at::empty({P, 2, N}, a.options().dtype(at::kFloat));
  TORCH_CHECK(mv_gemm_nt_bn_bwd(a.data_ptr(), b.data_ptr(), dz.data_ptr(), M, (int)N, (int)K, d2,
                                mp, xp, vp, partial.data_ptr<float>(), (int)bn, cur_stream(),
                                (int)dy2_stride, (int)H, (int)W),
              "gemm_nt_bn_bwd: launch failed");
  return partial;
}

}  // namespace

void bind_gemm(pybind11::module_& m) {
  namespace py = pybind11;
  m.def("gemm_nt", &gemm_nt, "C = A . B^T (bf16 MFMA) with optional fused BN statistics "
        "(C = None: statistics only)");
  m.def("gemm_apply_supported", &gemm_apply_supported, "gemm_nt_apply handles (N, K)");
  m.def("gram_stats", &gram_stats,
        "[1, 2, cout] BN statistics partials of x W^T from the Gram matrix x^T x and colsum(x)",
        py::arg("w"), py::arg("gram"), py::arg("xsum"), py::arg("shift") = py::none(),
        py::arg("m") = 1);
  m.def("fold_coeffs", &fold_coeffs,
        "{co [5, cout], xsum [cin]}: the BN fold's per-channel coefficients (mv_fold.hip)");
  m.def("fold_products", &fold_products,
        "{dW, bcat, badd}: the BN fold's small products (mv_fold.hip)");
  m.def("gemm_apply_dual_supported", &gemm_apply_dual_supported,
        "gemm_nt_apply_dual handles (N, K)");
  m.def("gemm_nt_apply_dual", &gemm_nt_apply_dual,
        "{y, mask}: the BN+add+ReLU apply GEMM with the shortcut conv + BN recomputed inside");
  m.def("gemm_dual_supported", &gemm_dual_supported, "gemm_dual_bias handles (K1, K2)");
  m.def("gemm_dual_bias_strided", &gemm_dual_bias_strided,
        "[A1 | x[:, :, ::s, ::s]] . B^T + badd without the strided copy; False if not covered");
  m.def("gemm_dual_bias", &gemm_dual_bias, "d = [a1 | a2] . b^T + badd (dual-source MFMA GEMM)");
  m.def("gemm_fold_dx_partials", &gemm_fold_dx_partials,
        "partial rows of gemm_fold_dx for (M, K1, K2) (-1: unsupported)");
  m.def("gemm_fold_dx", &gemm_fold_dx,
        "BN3-fold data gradient [a1|a2].b^T + badd with BN2's ReLU backward reduce -> partials");
  m.def("gemm_nt_apply", &gemm_nt_apply,
        "{y, mask}: relu(bf16(A . B^T) * scale + bias + res) from the GEMM epilogue "
        "(rscale/rbias: res = bf16(res * rscale + rbias), the shortcut BN's apply)",
        py::arg("a"), py::arg("b"), py::arg("res"), py::arg("scale"), py::arg("bias"),
        py::arg("rscale") = py::none(), py::arg("rbias") = py::none());
  m.def("gemm_nt_bn_bwd", &gemm_nt_bn_bwd,
        "1x1-conv data-gradient GEMM with the producing BN's add+ReLU backward reduce fused",
        py::arg("a"), py::arg("b"), py::arg("dz"), py::arg("dy2"), py::arg("mask"), py::arg("x"),
        py::arg("vec"), py::arg("bn") = 0, py::arg("dy2_stride") = 1, py::arg("H") = 1,
        py::arg("W") = 1);
  m.def("gemm_bwd_partials", &gemm_bwd_partials, "partial rows of gemm_nt_bn_bwd (-1: unsupported)",
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("bn") = 0);
  m.def("gemm_partials", &gemm_partials, "row tiles (statistics partial rows) of gemm_nt");
  m.def("gemm256_nt", &gemm256_nt, "C = A . B^T on the 256x256 glds-pipelined kernel alone");
  m.def("conv1x1_strided_stats", &conv1x1_strided_stats,
        "[y, (partials)] of a strided 1x1 conv on the 256x256 kernel (+ BN statistics), or None",
        py::arg("x"), py::arg("w"), py::arg("ds"), py::arg("shift") = py::none());
}
