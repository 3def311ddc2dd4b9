// mivod._mvk bindings: fused NHWC BatchNorm, SyncBatchNorm, pooling and the ResNet stem
// (mv_bn.h, mv_syncbn.h, mv_pool.h, mv_stem.h)
#include "mv_checks.h"
#include "mv_bn.h"
#include "mv_pool.h"
#include "mv_stem.h"
#include "mv_syncbn.h"

namespace {
using namespace mvc;

// optional tensor of x's shape, layout and dtype (residual, second gradient stream) -> pointer
const void* opt_same(const char* fn, const char* what, const OptTensor& t, const at::Tensor& x) {
  if (!given(t)) return nullptr;
  check_on(fn, what, *t, x, at::kBFloat16);
  TORCH_CHECK(t->sizes() == x.sizes() && t->strides() == x.strides(), fn, ": ", what,
              " must match the primary operand in shape and layout");
  return t->data_ptr();
}

// fp32 [P, 2, C] statistics / reduce partials (C < 0: any) -> P
int check_partials(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
                   int64_t C) {
  check_nd(fn, what, t, like, 3, at::kFloat);
  TORCH_CHECK(t.size(0) > 0 && t.size(0) < (int64_t(1) << 31) && t.size(1) == 2 &&
                  (C < 0 || t.size(2) == C),
              fn, ": ", what, " must be fp32 [P, 2, C] partials");
  return (int)t.size(0);
}

// both running statistics or neither
void running_ptrs(const char* fn, const OptTensor& mean, const OptTensor& var,
                  const at::Tensor& like, int64_t C, float** rm, float** rv) {
  *rm = vec_ptr_opt(fn, "running_mean", mean, like, C);
  *rv = vec_ptr_opt(fn, "running_var", var, like, C);
  TORCH_CHECK((*rm == nullptr) == (*rv == nullptr), fn, ": running_mean/var must both be given");
}

// Training forward, {y, vec} or (want_mask: relu + residual only) {y, vec, mask} with the
// [M, C/8] uint8 bitmask of y > 0 that backward mode 3 reads instead of y.  stats: the
// statistics come from the producing conv's epilogue as [P, 2, C] partials around rm.
std::vector<at::Tensor> bn_fwd(const char* fn, const at::Tensor& x, const OptTensor& gamma,
                               const OptTensor& beta, const OptTensor& running_mean,
                               const OptTensor& running_var, double momentum, double eps, bool relu,
                               const OptTensor& residual, bool want_mask, const at::Tensor* stats) {
  int64_t C;
  const int64_t M = check_act(fn, "x", x, x, &C);
  TORCH_CHECK(M > 0, fn, ": empty input");
  const int SP = stats ? check_partials(fn, "stats", *stats, x, C) : 0;
  const void* rp = opt_same(fn, "residual", residual, x);
  float *rm, *rv;
  running_ptrs(fn, running_mean, running_var, x, C, &rm, &rv);
  const float* gp = vec_ptr_opt(fn, "weight", gamma, x, C);
  const float* bp = vec_ptr_opt(fn, "bias", beta, x, C);
  TORCH_CHECK(!want_mask || (relu && rp), fn, ": the output bitmask needs relu and a residual");
  c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  at::Tensor vec = at::empty({4, C}, fo);  // save_mean, save_invstd, scale, bias
  at::Tensor y = at::empty_like(x);
  at::Tensor mask;
  if (want_mask) mask = at::empty({M, C / 8}, x.options().dtype(at::kByte));
  void* mp = want_mask ? mask.data_ptr() : nullptr;
  if (stats) {
    mv_bn_fwd_from_partials(x.data_ptr(), rp, y.data_ptr(), M, (int)C, rm, rv, gp, bp,
                            (float)momentum, (float)eps, relu, stats->data_ptr<float>(), SP,
                            vec[0].data_ptr<float>(), vec[1].data_ptr<float>(),
                            vec[2].data_ptr<float>(), vec[3].data_ptr<float>(), cur_stream(), mp);
  } else {
    const int P = mv_bn_partials(M, (int)C);
    at::Tensor partial = at::empty({(int64_t)P * 2 * C}, fo);
    mv_bn_fwd_train(x.data_ptr(), rp, y.data_ptr(), M, (int)C, rm, rv, gp, bp, (float)momentum,
                    (float)eps, relu, partial.data_ptr<float>(), P, vec[0].data_ptr<float>(),
                    vec[1].data_ptr<float>(), vec[2].data_ptr<float>(), vec[3].data_ptr<float>(),
                    cur_stream(), mp);
  }
  if (want_mask) return {y, vec, mask};
  return {y, vec};
}

at::Tensor bn_apply(at::Tensor x, at::Tensor scale, at::Tensor bias, bool relu,
                    c10::optional<at::Tensor> residual) {
  int64_t C;
  const int64_t M = check_act("bn_apply", "x", x, x, &C);
  const float* sp = vec_ptr("bn_apply", "scale", scale, x, C);
  const float* bp = vec_ptr("bn_apply", "bias", bias, x, C);
  const void* rp = opt_same("bn_apply", "residual", residual, x);
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  if (M == 0) return y;   // an empty batch (eval): nothing to launch
  mv_bn_apply(x.data_ptr(), rp, y.data_ptr(), M, (int)C, sp, bp, relu, cur_stream());
  return y;
}

// {y, partial}: y = relu(x * scale + bias) and [P, C] column-sum partials of y
std::vector<at::Tensor> bn_apply_colsum(at::Tensor x, at::Tensor scale, at::Tensor bias) {
  int64_t C;
  const int64_t M = check_act("bn_apply_colsum", "x", x, x, &C);
  TORCH_CHECK(M > 0, "bn_apply_colsum: empty input");
  const float* sp = vec_ptr("bn_apply_colsum", "scale", scale, x, C);
  const float* bp = vec_ptr("bn_apply_colsum", "bias", bias, x, C);
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  at::Tensor partial = at::empty({(int64_t)mv_bn_partials(M, (int)C), C},
                                 x.options().dtype(at::kFloat));
  const int P = mv_bn_apply_colsum(x.data_ptr(), y.data_ptr(), M, (int)C, sp, bp,
                                   partial.data_ptr<float>(), cur_stream());
  return {y, partial.narrow(0, 0, P)};
}

// statistics only: running-stat update + saved {mean, invstd, scale, bias}; no apply pass
at::Tensor bn_stats(at::Tensor x, c10::optional<at::Tensor> gamma, c10::optional<at::Tensor> beta,
                    c10::optional<at::Tensor> running_mean, c10::optional<at::Tensor> running_var,
                    double momentum, double eps) {
  int64_t C;
  const int64_t M = check_act("bn_stats", "x", x, x, &C);
  TORCH_CHECK(M > 0, "bn_stats: empty input");
  float *rm, *rv;
  running_ptrs("bn_stats", running_mean, running_var, x, C, &rm, &rv);
  const float* gp = vec_ptr_opt("bn_stats", "weight", gamma, x, C);
  const float* bp = vec_ptr_opt("bn_stats", "bias", beta, x, C);
  c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  const int P = mv_bn_partials(M, (int)C);
  at::Tensor partial = at::empty({(int64_t)P * 2 * C}, fo);
  at::Tensor vec = at::empty({4, C}, fo);
  mv_bn_fwd_train(x.data_ptr(), nullptr, nullptr, M, (int)C, rm, rv, gp, bp, (float)momentum,
                  (float)eps, false, partial.data_ptr<float>(), P, vec[0].data_ptr<float>(),
                  vec[1].data_ptr<float>(), vec[2].data_ptr<float>(), vec[3].data_ptr<float>(),
                  cur_stream());
  return vec;
}

// statistics of x[:, :, ::s, ::s] without the strided copy -> [4, C] {mean, invstd, ...}
at::Tensor bn_stats_strided(at::Tensor x, int64_t stride) {
  check_chlast("bn_stats_strided", "x", x, x, 8);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(stride >= 1 && stride < 65536 && H < 65536 && W < 65536,
              "bn_stats_strided: bad stride / size");
  const int64_t M = N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  TORCH_CHECK(M > 0 && M < (int64_t(1) << 32), "bn_stats_strided: empty or too large");
  c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  const int P = mv_bn_partials(M, (int)C);
  at::Tensor partial = at::empty({(int64_t)P * 2 * C}, fo);
  at::Tensor vec = at::empty({4, C}, fo);
  mv_bn_stats_strided(x.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)stride,
                      partial.data_ptr<float>(), P, vec[0].data_ptr<float>(),
                      vec[1].data_ptr<float>(), vec[2].data_ptr<float>(), vec[3].data_ptr<float>(),
                      cur_stream());
  return vec;
}

// returns {dx, dgamma, dbeta, dz}; dz defined only for modes 2 and 3 (residual branch grad)
std::vector<at::Tensor> bn_bwd(int64_t mode, at::Tensor dy, at::Tensor x,
                               c10::optional<at::Tensor> y, at::Tensor vec,
                               c10::optional<at::Tensor> gamma, bool need_affine_grad,
                               c10::optional<at::Tensor> dy2, int64_t dy2_stride) {
  int64_t C, C2;
  check_act("bn_bwd", "dy", dy, dy, &C2);
  const int64_t M = check_act("bn_bwd", "x", x, dy, &C);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(),
              "bn_bwd: dy must match x in shape and layout");
  TORCH_CHECK(M > 0, "bn_bwd: empty input");
  TORCH_CHECK(mode >= 0 && mode <= 3, "bn_bwd: bad mode");
  const float* vp = vec_ptr("bn_bwd", "vec", vec, x, 4 * C);
  const float* gp = vec_ptr_opt("bn_bwd", "weight", gamma, x, C);
  const void* yp = nullptr;
  if (mode == 2) {
    yp = opt_same("bn_bwd", "y", y, x);
    TORCH_CHECK(yp, "bn_bwd: mode 2 needs the saved output");
  } else if (mode == 3) {
    TORCH_CHECK(given(y), "bn_bwd: mode 3 needs the forward's [M, C/8] uint8 bitmask");
    yp = vec_ptr<uint8_t>("bn_bwd", "y", *y, x, M * (C / 8));
  }
  const void* dy2p = nullptr;
  if (given(dy2)) {
    TORCH_CHECK(mode >= 2, "bn_bwd: a second gradient stream is supported for modes 2 and 3 only");
    TORCH_CHECK(dy2_stride >= 1, "bn_bwd: bad dy2 stride");
    if (dy2_stride == 1) {
      dy2p = opt_same("bn_bwd", "dy2", dy2, x);
    } else {
      const int64_t s = dy2_stride;
      TORCH_CHECK(M < (int64_t(1) << 32), "bn_bwd: strided dy2 needs fewer than 2^32 rows");
      check_chlast("bn_bwd", "dy2", *dy2, x);
      TORCH_CHECK(x.dim() == 4 && dy2->size(0) == x.size(0) && dy2->size(1) == x.size(1) &&
                      dy2->size(2) == (x.size(2) + s - 1) / s &&
                      dy2->size(3) == (x.size(3) + s - 1) / s,
                  "bn_bwd: strided dy2 must be [N, C, ceil(H/s), ceil(W/s)]");
      dy2p = dy2->data_ptr();
    }
  }
  c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  const int P = mv_bn_partials(M, (int)C);
  at::Tensor partial = at::empty({(int64_t)P * 2 * C}, fo);
  at::Tensor work = at::empty({5, C}, fo);  // dgamma, dbeta, a, b, c
  at::Tensor dx = at::empty_like(x);
  at::Tensor dz;
  if (mode >= 2) dz = at::empty_like(x);
  mv_bn_bwd((int)mode, dy.data_ptr(), dy2p, x.data_ptr(), yp, mode >= 2 ? dz.data_ptr() : nullptr,
            dx.data_ptr(), M, (int)C, vp, vp + C, gp, vp + 2 * C, vp + 3 * C,
            work[0].data_ptr<float>(), work[1].data_ptr<float>(), partial.data_ptr<float>(), P,
            work[2].data_ptr<float>(), work[3].data_ptr<float>(), work[4].data_ptr<float>(),
            dy2p ? (int)dy2_stride : 1, x.dim() == 4 ? (int)x.size(2) : 1,
            x.dim() == 4 ? (int)x.size(3) : 1, cur_stream());
  at::Tensor dg, db;
  if (need_affine_grad) {
    dg = work[0];
    db = work[1];
  }
  return {dx, dg, db, dz};
}

// {4, C} saved statistics (mean, invstd, scale, bias) + running-stat update from [P, 2, C]
// GEMM-epilogue partials of an M-row activation; no apply pass
at::Tensor bn_finalize(at::Tensor stats, c10::optional<at::Tensor> gamma,
                       c10::optional<at::Tensor> beta, c10::optional<at::Tensor> running_mean,
                       c10::optional<at::Tensor> running_var, double momentum, double eps,
                       int64_t M) {
  const int P = check_partials("bn_finalize", "stats", stats, stats, -1);
  TORCH_CHECK(M > 0, "bn_finalize: M must be positive");
  const int64_t C = stats.size(2);
  float *rm, *rv;
  running_ptrs("bn_finalize", running_mean, running_var, stats, C, &rm, &rv);
  const float* gp = vec_ptr_opt("bn_finalize", "weight", gamma, stats, C);
  const float* bp = vec_ptr_opt("bn_finalize", "bias", beta, stats, C);
  c10::DeviceGuard guard(stats.device());
  at::Tensor vec = at::empty({4, C}, stats.options());
  mv_bn_fwd_from_partials(nullptr, nullptr, nullptr, M, (int)C, rm, rv, gp, bp, (float)momentum,
                          (float)eps, false, stats.data_ptr<float>(), P, vec[0].data_ptr<float>(),
                          vec[1].data_ptr<float>(), vec[2].data_ptr<float>(),
                          vec[3].data_ptr<float>(), cur_stream());
  return vec;
}

// Finalize of a backward reduce: [5, C] fp32 = (dgamma, dbeta, ca, cb, cc) from [P, 2, C]
// partials, and (dz, x, dx given) the BN's input gradient dx = ca * dz + cb * x + cc.
// vp: the saved [4, C]; part / P: checked by the caller.
at::Tensor bwd_finalize(const void* dz, const void* x, void* dx, int64_t M, int64_t C,
                        const float* vp, const float* gp, const at::Tensor& part, int P) {
  at::Tensor work = at::empty({5, C}, part.options());
  mv_bn_bwd_from_partials(dz, x, dx, M, (int)C, vp, vp + C, gp, vp + 2 * C, vp + 3 * C,
                          work[0].data_ptr<float>(), work[1].data_ptr<float>(),
                          part.data_ptr<float>(), P, work[2].data_ptr<float>(),
                          work[3].data_ptr<float>(), work[4].data_ptr<float>(), cur_stream());
  return work;
}

// [5, C] fp32 = (dgamma, dbeta, ca, cb, cc) from a GEMM-epilogue reduce's partials, with
// the BN's input gradient dx = ca * dz + cb * x + cc (per channel) left to the caller
at::Tensor bn_bwd_coeffs(at::Tensor vec, c10::optional<at::Tensor> gamma, at::Tensor partial,
                         int64_t M) {
  const int64_t C = vec.numel() / 4;
  const float* vp = vec_ptr("bn_bwd_coeffs", "vec", vec, vec, 4 * C);
  const int P = check_partials("bn_bwd_coeffs", "partial", partial, vec, C);
  const float* gp = vec_ptr_opt("bn_bwd_coeffs", "weight", gamma, vec, C);
  TORCH_CHECK(M > 0, "bn_bwd_coeffs: M must be positive");
  c10::DeviceGuard guard(vec.device());
  return bwd_finalize(nullptr, nullptr, nullptr, M, C, vp, gp, partial, P);
}

// {dx, dgamma, dbeta} from a GEMM-epilogue reduce (gemm_nt_bn_bwd)
std::vector<at::Tensor> bn_bwd_from_partials(at::Tensor dz, at::Tensor x, at::Tensor vec,
                                             c10::optional<at::Tensor> gamma,
                                             bool need_affine_grad, at::Tensor partial) {
  int64_t C, C2;
  check_act("bn_bwd_from_partials", "dz", dz, dz, &C2);
  const int64_t M = check_act("bn_bwd_from_partials", "x", x, dz, &C);
  TORCH_CHECK(dz.sizes() == x.sizes() && dz.strides() == x.strides(),
              "bn_bwd_from_partials: dz must match x in shape and layout");
  const float* vp = vec_ptr("bn_bwd_from_partials", "vec", vec, x, 4 * C);
  const int P = check_partials("bn_bwd_from_partials", "partial", partial, x, C);
  const float* gp = vec_ptr_opt("bn_bwd_from_partials", "weight", gamma, x, C);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  at::Tensor work = bwd_finalize(dz.data_ptr(), x.data_ptr(), dx.data_ptr(), M, C, vp, gp,
                                 partial, P);
  at::Tensor dg, db;
  if (need_affine_grad) {
    dg = work[0];
    db = work[1];
  }
  return {dx, dg, db};
}

// ---------------------------------------------------------------------------
// SyncBatchNorm (mv_syncbn.h): the local passes and the kernels around the two collectives
// ---------------------------------------------------------------------------
// int32 [N, 3C + 4] gathered statistics records -> N, sets *C
int check_records(const char* fn, const at::Tensor& recs, const at::Tensor& like, int64_t* C) {
  check_nd(fn, "records", recs, like, 2, at::kInt);
  const int64_t w = recs.size(1);
  TORCH_CHECK(recs.size(0) > 0 && recs.size(0) < (int64_t(1) << 20) && w > 4 && (w - 4) % 24 == 0,
              fn, ": records must be int32 [N, 3 C + 4] with C % 8 == 0");
  *C = (w - 4) / 3;
  return (int)recs.size(0);
}

// {record int32 [3C + 4], P}: this rank's statistics pass around shift and its record;
// P = the [2][C] partial rows the pass produced
std::tuple<at::Tensor, int64_t> syncbn_stats(at::Tensor x, c10::optional<at::Tensor> shift) {
  const char* fn = "syncbn_stats";
  int64_t C;
  const int64_t M = check_act(fn, "x", x, x, &C);
  TORCH_CHECK(M > 0, fn, ": empty input");
  const float* sp = vec_ptr_opt(fn, "shift", shift, x, C);
  c10::DeviceGuard guard(x.device());
  const int P = mv_bn_partials(M, (int)C);
  at::Tensor partial = at::empty({(int64_t)P * 2 * C}, x.options().dtype(at::kFloat));
  at::Tensor rec = at::empty({mv_syncbn_record_words((int)C)}, x.options().dtype(at::kInt));
  const int pa = mv_bn_stats_pass(x.data_ptr(), M, (int)C, sp, partial.data_ptr<float>(), P,
                                  cur_stream());
  mv_syncbn_record(partial.data_ptr<float>(), pa, M, (int)C, sp, rec.data_ptr<int32_t>(),
                   cur_stream());
  return {rec, (int64_t)pa};
}

// records of every rank in rank order -> {vec [4, C], count int64 [1]} + running-stat update
std::vector<at::Tensor> syncbn_merge_impl(const char* fn, const at::Tensor& recs,
                                          const OptTensor& gamma, const OptTensor& beta,
                                          const OptTensor& running_mean,
                                          const OptTensor& running_var, double momentum,
                                          double eps) {
  int64_t C;
  const int N = check_records(fn, recs, recs, &C);
  float *rm, *rv;
  running_ptrs(fn, running_mean, running_var, recs, C, &rm, &rv);
  const float* gp = vec_ptr_opt(fn, "weight", gamma, recs, C);
  const float* bp = vec_ptr_opt(fn, "bias", beta, recs, C);
  c10::DeviceGuard guard(recs.device());
  at::Tensor vec = at::empty({4, C}, recs.options().dtype(at::kFloat));
  at::Tensor count = at::empty({1}, recs.options().dtype(at::kLong));
  mv_syncbn_merge(recs.data_ptr<int32_t>(), N, (int)C, rm, rv, gp, bp, (float)momentum,
                  (float)eps, vec.data_ptr<float>(), count.data_ptr<int64_t>(), cur_stream());
  return {vec, count};
}

// merge + apply: {y, vec, count} or (want_mask: relu + residual only) {y, vec, count, mask}
std::vector<at::Tensor> syncbn_fwd(at::Tensor x, at::Tensor recs, c10::optional<at::Tensor> gamma,
                                   c10::optional<at::Tensor> beta,
                                   c10::optional<at::Tensor> running_mean,
                                   c10::optional<at::Tensor> running_var, double momentum,
                                   double eps, bool relu, c10::optional<at::Tensor> residual,
                                   bool want_mask) {
  const char* fn = "syncbn_fwd";
  int64_t C, CR;
  const int64_t M = check_act(fn, "x", x, x, &C);
  TORCH_CHECK(M > 0, fn, ": empty input");
  check_records(fn, recs, x, &CR);
  TORCH_CHECK(CR == C, fn, ": records are for ", CR, " channels, x has ", C);
  const void* rp = opt_same(fn, "residual", residual, x);
  TORCH_CHECK(!want_mask || (relu && rp), fn, ": the output bitmask needs relu and a residual");
  std::vector<at::Tensor> out =
      syncbn_merge_impl(fn, recs, gamma, beta, running_mean, running_var, momentum, eps);
  c10::DeviceGuard guard(x.device());
  const float* vp = out[0].data_ptr<float>();
  at::Tensor y = at::empty_like(x);
  at::Tensor mask;
  if (want_mask) mask = at::empty({M, C / 8}, x.options().dtype(at::kByte));
  mv_bn_apply(x.data_ptr(), rp, y.data_ptr(), M, (int)C, vp + 2 * C, vp + 3 * C, relu,
              cur_stream(), want_mask ? mask.data_ptr() : nullptr);
  if (want_mask) return {y, out[0], out[1], mask};
  return {y, out[0], out[1]};
}

// The backward's local half, {tot [2, C], dgamma, dbeta, dz}: the reduce pass of bn_bwd's
// modes, this rank's affine gradients and its (sum dz, sum dz (x - mean)) for the sum over
// ranks; dz defined for modes 2 and 3
std::vector<at::Tensor> syncbn_bwd_reduce(int64_t mode, at::Tensor dy, at::Tensor x,
                                          c10::optional<at::Tensor> y, at::Tensor vec,
                                          bool need_affine_grad) {
  const char* fn = "syncbn_bwd_reduce";
  int64_t C, C2;
  check_act(fn, "dy", dy, dy, &C2);
  const int64_t M = check_act(fn, "x", x, dy, &C);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), fn,
              ": dy must match x in shape and layout");
  TORCH_CHECK(M > 0, fn, ": empty input");
  TORCH_CHECK(mode >= 0 && mode <= 3, fn, ": bad mode");
  const float* vp = vec_ptr(fn, "vec", vec, x, 4 * C);
  const void* yp = nullptr;
  if (mode == 2) {
    yp = opt_same(fn, "y", y, x);
    TORCH_CHECK(yp, fn, ": mode 2 needs the saved output");
  } else if (mode == 3) {
    TORCH_CHECK(given(y), fn, ": mode 3 needs the forward's [M, C/8] uint8 bitmask");
    yp = vec_ptr<uint8_t>(fn, "y", *y, x, M * (C / 8));
  }
  c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  const int P = mv_bn_partials(M, (int)C);
  at::Tensor partial = at::empty({(int64_t)P * 2 * C}, fo);
  at::Tensor tot = at::empty({2, C}, fo);
  at::Tensor dg, db, dz;
  if (need_affine_grad) {
    dg = at::empty({C}, fo);
    db = at::empty({C}, fo);
  }
  if (mode >= 2) dz = at::empty_like(x);
  const int pa = mv_bn_bwd_reduce_pass((int)mode, dy.data_ptr(), nullptr, x.data_ptr(), yp,
                                       mode >= 2 ? dz.data_ptr() : nullptr, M, (int)C, vp,
                                       vp + 2 * C, vp + 3 * C, partial.data_ptr<float>(), P, 1, 1,
                                       1, cur_stream());
  mv_syncbn_bwd_local(partial.data_ptr<float>(), pa, (int)C, vp + C,
                      need_affine_grad ? dg.data_ptr<float>() : nullptr,
                      need_affine_grad ? db.data_ptr<float>() : nullptr, tot.data_ptr<float>(),
                      cur_stream());
  return {tot, dg, db, dz};
}

// The backward's global half: dx from the totals summed over ranks and the forward's global
// count; d = dy (modes 0, 1) or the reduce's dz (modes 2, 3)
at::Tensor syncbn_bwd_dx(int64_t mode, at::Tensor d, at::Tensor x, at::Tensor vec,
                         c10::optional<at::Tensor> gamma, at::Tensor tot, at::Tensor count) {
  const char* fn = "syncbn_bwd_dx";
  int64_t C, C2;
  check_act(fn, "d", d, d, &C2);
  const int64_t M = check_act(fn, "x", x, d, &C);
  TORCH_CHECK(d.sizes() == x.sizes() && d.strides() == x.strides(), fn,
              ": d must match x in shape and layout");
  TORCH_CHECK(mode >= 0 && mode <= 3, fn, ": bad mode");
  const float* vp = vec_ptr(fn, "vec", vec, x, 4 * C);
  const float* gp = vec_ptr_opt(fn, "weight", gamma, x, C);
  const float* tp = vec_ptr(fn, "tot", tot, x, 2 * C);
  const int64_t* cp = vec_ptr<int64_t>(fn, "count", count, x, 1);
  c10::DeviceGuard guard(x.device());
  at::Tensor co = at::empty({3, C}, x.options().dtype(at::kFloat));
  at::Tensor dx = at::empty_like(x);
  mv_syncbn_bwd_coeffs(tp, cp, (int)C, vp, vp + C, gp, co[0].data_ptr<float>(),
                       co[1].data_ptr<float>(), co[2].data_ptr<float>(), cur_stream());
  mv_bn_bwd_dx_pass((int)mode, d.data_ptr(), x.data_ptr(), dx.data_ptr(), M, (int)C, vp + 2 * C,
                    vp + 3 * C, co[0].data_ptr<float>(), co[1].data_ptr<float>(),
                    co[2].data_ptr<float>(), cur_stream());
  return dx;
}

// ---------------------------------------------------------------------------
// NHWC pooling
// ---------------------------------------------------------------------------
std::vector<at::Tensor> maxpool_fwd(at::Tensor x, c10::optional<at::Tensor> scale,
                                    c10::optional<at::Tensor> bias, bool relu, int64_t k,
                                    int64_t s, int64_t p) {
  check_chlast("maxpool_fwd", "x", x, x, 8);
  TORCH_CHECK(k >= 1 && k * k <= 255 && s >= 1 && p >= 0 && 2 * p <= k,
              "maxpool_fwd: bad window");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
  TORCH_CHECK(OH > 0 && OW > 0, "maxpool_fwd: empty output");
  TORCH_CHECK(N * OH * OW * (C / 8) < (int64_t(1) << 32),
              "maxpool_fwd: the kernel indexes N*OH*OW*C/8 lanes in 32 bits");
  const float* sp = vec_ptr_opt("maxpool_fwd", "scale", scale, x, C);
  const float* bp = sp ? vec_ptr_opt("maxpool_fwd", "bias", bias, x, C) : nullptr;
  TORCH_CHECK(!sp || bp, "maxpool_fwd: scale needs bias");
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty({N, C, OH, OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor idx = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
  mv_maxpool_fwd(x.data_ptr(), sp, bp, relu, y.data_ptr(), idx.data_ptr<uint8_t>(), (int)N,
                 (int)H, (int)W, (int)C, (int)OH, (int)OW, (int)k, (int)s, (int)p, cur_stream());
  return {y, idx};
}

// optional second pooled gradient stream of dy's shape -> pointer
const void* pool_dy2(const char* fn, const OptTensor& dy2, const at::Tensor& dy) {
  if (!given(dy2)) return nullptr;
  check_chlast(fn, "dy2", *dy2, dy, 8);
  TORCH_CHECK(dy2->sizes() == dy.sizes(), fn, ": dy2 must have dy's shape");
  return dy2->data_ptr();
}

at::Tensor maxpool_bwd(at::Tensor dy, c10::optional<at::Tensor> dy2, at::Tensor idx, int64_t H,
                       int64_t W, int64_t k, int64_t s, int64_t p) {
  check_chlast("maxpool_bwd", "dy", dy, dy, 8);
  const int64_t N = dy.size(0), C = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  TORCH_CHECK(OH == (H + 2 * p - k) / s + 1 && OW == (W + 2 * p - k) / s + 1,
              "maxpool_bwd: output size does not match the window");
  const uint8_t* ip = vec_ptr<uint8_t>("maxpool_bwd", "idx", idx, dy, dy.numel());
  TORCH_CHECK(N * H * W * (C / 8) < (int64_t(1) << 32),
              "maxpool_bwd: the kernel indexes N*H*W*C/8 lanes in 32 bits");
  const void* d2 = pool_dy2("maxpool_bwd", dy2, dy);
  c10::DeviceGuard guard(dy.device());
  at::Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  mv_maxpool_bwd(dy.data_ptr(), d2, ip, dx.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)OH,
                 (int)OW, (int)k, (int)s, (int)p, cur_stream());
  return dx;
}

// [5, C] fp32 {dgamma, dbeta, ca, cb, cc} of the BN+ReLU in front of a maxpool, from a reduce
// over the pooled tensors (dy, dy2, the pooled output y); M = the BN's element rows
at::Tensor pool_bn_coefs(const at::Tensor& dy, const void* d2, const at::Tensor& y,
                         const float* vp, const float* gp, int64_t M) {
  const int64_t C = dy.size(1);
  at::Tensor part = at::empty({(int64_t)mv_pool_bn_partials(), 2, C},
                              dy.options().dtype(at::kFloat));
  mv_pool_bn_reduce(dy.data_ptr(), d2, y.data_ptr(), vp, vp + 2 * C, vp + 3 * C,
                    part.data_ptr<float>(), dy.numel() / C, (int)C, cur_stream());
  return bwd_finalize(nullptr, nullptr, nullptr, M, C, vp, gp, part, (int)part.size(0));
}

// {dx, dgamma, dbeta}: maxpool(3, 2, 1) backward fused with the backward of the BN+ReLU that
// produced its input z (ResNet stem): y = the pooled output, vec = the BN's saved [4, C]
std::vector<at::Tensor> maxpool_bn_bwd(at::Tensor dy, c10::optional<at::Tensor> dy2,
                                       at::Tensor idx, at::Tensor y, at::Tensor z, at::Tensor vec,
                                       c10::optional<at::Tensor> gamma) {
  const char* fn = "maxpool_bn_bwd";
  check_chlast(fn, "dy", dy, dy, 8);
  check_chlast(fn, "y", y, dy, 8);
  check_chlast(fn, "z", z, dy, 8);
  const int64_t N = dy.size(0), C = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  const int64_t H = z.size(2), W = z.size(3);
  TORCH_CHECK(y.sizes() == dy.sizes() && z.size(0) == N && z.size(1) == C && H % 2 == 0 &&
                  W % 2 == 0 && OH == H / 2 && OW == W / 2 && C <= 256,
              "maxpool_bn_bwd: needs a 3x3 / 2 / pad-1 pool of an even-sized input, C % 8 == 0, C <= 256");
  const uint8_t* ip = vec_ptr<uint8_t>(fn, "idx", idx, dy, dy.numel());
  TORCH_CHECK(N * H * W * (C / 8) < (int64_t(1) << 32), "maxpool_bn_bwd: too large");
  const float* vp = vec_ptr(fn, "vec", vec, dy, 4 * C);
  const float* gp = vec_ptr_opt(fn, "weight", gamma, dy, C);
  const void* d2 = pool_dy2(fn, dy2, dy);
  c10::DeviceGuard guard(dy.device());
  at::Tensor work = pool_bn_coefs(dy, d2, y, vp, gp, N * H * W);
  at::Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  TORCH_CHECK(mv_maxpool_bn_bwd(dy.data_ptr(), d2, ip, z.data_ptr(), vp + 2 * C, vp + 3 * C,
                                work[2].data_ptr<float>(), work[3].data_ptr<float>(),
                                work[4].data_ptr<float>(), dx.data_ptr(), (int)N, (int)H, (int)W,
                                (int)C, (int)OH, (int)OW, cur_stream()),
              "maxpool_bn_bwd: launch failed");
  return {dx, work[0], work[1]};
}

at::Tensor gap_fwd(at::Tensor x) {
  check_chlast("gap_fwd", "x", x, x, 8);
  c10::DeviceGuard guard(x.device());
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  at::Tensor y = at::empty({N, C}, x.options());
  mv_gap_fwd(x.data_ptr(), y.data_ptr(), (int)N, (int)HW, (int)C, cur_stream());
  return y;
}

at::Tensor gap_bwd(at::Tensor dy, int64_t H, int64_t W) {
  check_nd("gap_bwd", "dy", dy, dy, 2);
  const int64_t N = dy.size(0), C = dy.size(1);
  TORCH_CHECK(C % 8 == 0, "gap_bwd: dy must be [N, C] with C % 8 == 0");
  TORCH_CHECK(N * H * W * (C / 8) < (int64_t(1) << 32),
              "gap_bwd: the kernel indexes N*H*W*C/8 lanes in 32 bits");
  c10::DeviceGuard guard(dy.device());
  at::Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  mv_gap_bwd(dy.data_ptr(), dx.data_ptr(), (int)N, (int)(H * W), (int)C, cur_stream());
  return dx;
}

at::Tensor pad_channels(at::Tensor x, int64_t cout) {
  check_chlast("pad_channels", "x", x, x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C >= 1 && C <= 8 && cout >= C && cout <= 8, "pad_channels: need C <= cout <= 8");
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty({N, cout, H, W},
                           x.options().memory_format(at::MemoryFormat::ChannelsLast));
  mv_pad_channels(x.data_ptr(), y.data_ptr(), N * H * W, (int)C, (int)cout, cur_stream());
  return y;
}

// ---------------------------------------------------------------------------
// ResNet stem (7x7 / 2 / pad 3 on a 3- or 4-channel 224x224 NHWC image)
// ---------------------------------------------------------------------------
int64_t check_stem_x(const char* fn, const at::Tensor& x) {
  check_chlast(fn, "x", x, x);
  const int64_t N = x.size(0);
  TORCH_CHECK((x.size(1) == 4 || x.size(1) == 3) && x.size(2) == 224 && x.size(3) == 224, fn,
              ": x must be [N, 3 or 4, 224, 224]");
  TORCH_CHECK(N > 0 && N * 112 < (int64_t(1) << 31), fn, ": bad batch");
  return N;
}

// {z [N, 64, 112, 112] channels_last bf16, partial [P, 2, 64]}: the stem conv with BN
// statistics around shift
std::vector<at::Tensor> stem_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> shift,
                                 int64_t grid) {
  const int64_t N = check_stem_x("stem_fwd", x);
  check_chlast("stem_fwd", "w", w, x);
  TORCH_CHECK(w.sizes() == at::IntArrayRef({64, 4, 7, 7}), "stem_fwd: w must be [64, 4, 7, 7]");
  const float* sp = vec_ptr_opt("stem_fwd", "shift", shift, x, 64);
  // grid > 0: a non-default persistent grid (tests); any size >= 1 is valid — the
  // kernel's row loop and the partial rows follow the grid
  TORCH_CHECK(grid >= 0 && grid <= (int64_t(1) << 20), "stem_fwd: bad grid");
  c10::DeviceGuard guard(x.device());
  at::Tensor z = at::empty({N, 64, 112, 112},
                           x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int g = grid > 0 ? (int)grid : mv_stem_partials((int)N);
  at::Tensor part = at::empty({(int64_t)g, 2, 64}, x.options().dtype(at::kFloat));
  mv_stem_fwd(x.data_ptr(), w.data_ptr(), z.data_ptr(), sp, part.data_ptr<float>(), (int)N,
              cur_stream(), g, (int)x.size(1));
  return {z, part};
}

// dw [64, 4, 7, 7] channels_last bf16: the stem conv's weight gradient (mv_stem.hip)
at::Tensor stem_wgrad(at::Tensor x, at::Tensor dz) {
  const int64_t N = check_stem_x("stem_wgrad", x);
  check_chlast("stem_wgrad", "dz", dz, x);
  TORCH_CHECK(dz.sizes() == at::IntArrayRef({N, 64, 112, 112}),
              "stem_wgrad: dz must be [N, 64, 112, 112]");
  c10::DeviceGuard guard(x.device());
  at::Tensor work = at::empty({(int64_t)mv_stem_wgrad_blocks((int)N) * 64 * 224},
                              x.options().dtype(at::kFloat));
  at::Tensor dw = at::empty({64, 4, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  mv_stem_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), work.data_ptr<float>(), (int)N,
                cur_stream(), (int)x.size(1));
  return dw;
}

// {dw, dgamma, dbeta}: the ResNet stem's maxpool + BN+ReLU backward and its conv's weight
// gradient in one pass over the rows (mv_stem.hip, MvStemPoolBwd): the full-resolution dz is
// never written.  x: the stem input, z: the conv output, y / idx: the pooled output and its
// window argmax, vec: the BN's saved [4, 64]; dy (+ dy2): the pooled gradients.
std::vector<at::Tensor> stem_wgrad_pool_bn(at::Tensor x, at::Tensor dy,
                                           c10::optional<at::Tensor> dy2, at::Tensor idx,
                                           at::Tensor y, at::Tensor z, at::Tensor vec,
                                           c10::optional<at::Tensor> gamma) {
  const char* fn = "stem_wgrad_pool_bn";
  const int64_t N = check_stem_x(fn, x);
  check_chlast(fn, "z", z, x, 8);
  check_chlast(fn, "dy", dy, x, 8);
  check_chlast(fn, "y", y, x, 8);
  TORCH_CHECK(z.sizes() == at::IntArrayRef({N, 64, 112, 112}),
              "stem_wgrad_pool_bn: z must be [N, 64, 112, 112]");
  TORCH_CHECK(dy.sizes() == at::IntArrayRef({N, 64, 56, 56}) && y.sizes() == dy.sizes(),
              "stem_wgrad_pool_bn: dy / y must be [N, 64, 56, 56]");
  const uint8_t* ip = vec_ptr<uint8_t>(fn, "idx", idx, x, dy.numel());
  const float* vp = vec_ptr(fn, "vec", vec, x, 4 * 64);
  const float* gp = vec_ptr_opt(fn, "weight", gamma, x, 64);
  const void* d2 = pool_dy2(fn, dy2, dy);
  c10::DeviceGuard guard(x.device());
  at::Tensor coef = pool_bn_coefs(dy, d2, y, vp, gp, N * 112 * 112);
  at::Tensor work = at::empty({(int64_t)mv_stem_wgrad_blocks((int)N) * 64 * 224},
                              x.options().dtype(at::kFloat));
  at::Tensor dw = at::empty({64, 4, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  MvStemPoolBwd pb{z.data_ptr(), dy.data_ptr(), d2, ip, vp + 2 * 64, vp + 3 * 64,
                   coef[2].data_ptr<float>(), coef[3].data_ptr<float>(),
                   coef[4].data_ptr<float>()};
  mv_stem_wgrad_pool_bn(x.data_ptr(), pb, dw.data_ptr(), work.data_ptr<float>(), (int)N,
                        cur_stream(), (int)x.size(1));
  return {dw, coef[0], coef[1]};
}

}  // namespace

void bind_bn(pybind11::module_& m) {
  using Opt = c10::optional<at::Tensor>;
  m.def("bn_fwd_train",
        [](at::Tensor x, Opt gamma, Opt beta, Opt running_mean, Opt running_var, double momentum,
           double eps, bool relu, Opt residual) {
          return bn_fwd("bn_fwd_train", x, gamma, beta, running_mean, running_var, momentum, eps,
                        relu, residual, false, nullptr);
        },
        "fused NHWC BN(+add)(+ReLU) training forward");
  m.def("bn_fwd_train_mask",
        [](at::Tensor x, Opt gamma, Opt beta, Opt running_mean, Opt running_var, double momentum,
           double eps, at::Tensor residual) {
          return bn_fwd("bn_fwd_train_mask", x, gamma, beta, running_mean, running_var, momentum,
                        eps, true, residual, true, nullptr);
        },
        "fused NHWC BN+add+ReLU training forward that also returns the backward bitmask");
  m.def("bn_apply", &bn_apply, "NHWC y = act(x*scale + bias (+res))");
  m.def("bn_fwd_train_stats",
        [](at::Tensor x, at::Tensor stats, Opt gamma, Opt beta, Opt running_mean, Opt running_var,
           double momentum, double eps, bool relu, Opt residual, bool want_mask) {
          return bn_fwd("bn_fwd_train_stats", x, gamma, beta, running_mean, running_var, momentum,
                        eps, relu, residual, want_mask, &stats);
        },
        "fused BN(+add)(+ReLU) forward from the conv epilogue's statistics partials");
  m.def("bn_bwd", &bn_bwd, "fused NHWC BN(+add)(+ReLU) backward (+ second grad stream)");
  m.def("bn_stats", &bn_stats, "NHWC BN training statistics only -> [4, C]");
  m.def("bn_stats_strided", &bn_stats_strided,
        "statistics of x[:, :, ::s, ::s] (no strided copy) -> [4, C] {mean, invstd, ...}");
  m.def("bn_apply_colsum", &bn_apply_colsum,
        "{y, [P, C] partials}: relu(x*scale + bias) with column sums of y");
  m.def("bn_finalize", &bn_finalize, "BN statistics finalize from [P, 2, C] partials -> [4, C]");
  m.def("bn_bwd_coeffs", &bn_bwd_coeffs,
        "BN backward finalize only: [5, C] = (dgamma, dbeta, ca, cb, cc) from partials");
  m.def("bn_bwd_from_partials", &bn_bwd_from_partials,
        "BN backward finalize + dx from GEMM-epilogue partials -> (dx, dgamma, dbeta)");
  // SyncBatchNorm has a namespace of its own: mivod._mvk._syncbn
  pybind11::module_ sb = m.def_submodule(
      "_syncbn", "SyncBatchNorm: the local BN passes and the kernels around its two collectives");
  sb.def("syncbn_stats", &syncbn_stats,
        "{record int32 [3C + 4], P}: local statistics pass + this rank's SyncBatchNorm record",
        pybind11::arg("x"), pybind11::arg("shift") = pybind11::none());
  sb.def("syncbn_merge",
        [](at::Tensor recs, Opt gamma, Opt beta, Opt running_mean, Opt running_var, double momentum,
           double eps) {
          return syncbn_merge_impl("syncbn_merge", recs, gamma, beta, running_mean, running_var,
                                   momentum, eps);
        },
        "gathered [N, 3C + 4] records -> {vec [4, C], count int64 [1]} + running-stat update");
  sb.def("syncbn_fwd", &syncbn_fwd,
        "SyncBatchNorm forward after the allgather: merge + apply -> {y, vec, count[, mask]}");
  sb.def("syncbn_bwd_reduce", &syncbn_bwd_reduce,
        "SyncBatchNorm backward, local half -> {tot [2, C], dgamma, dbeta, dz}");
  sb.def("syncbn_bwd_dx", &syncbn_bwd_dx,
        "SyncBatchNorm backward, global half: dx from the summed totals and the global count");
  m.def("maxpool_fwd", &maxpool_fwd, "NHWC maxpool with fused affine+ReLU prologue -> (y, idx)");
  m.def("maxpool_bwd", &maxpool_bwd, "NHWC maxpool backward (gather, + second grad stream)");
  m.def("maxpool_bn_bwd", &maxpool_bn_bwd,
        "{dx, dgamma, dbeta}: maxpool(3,2,1) backward fused with its producer BN+ReLU backward");
  m.def("gap_fwd", &gap_fwd, "NHWC global average pool -> [N, C]");
  m.def("gap_bwd", &gap_bwd, "NHWC global average pool backward");
  m.def("pad_channels", &pad_channels, "NHWC zero channel padding C -> cout (<= 8)");
  m.def("stem_wgrad", &stem_wgrad, "ResNet stem conv weight gradient on MFMA (mv_stem.hip)");
  m.def("stem_wgrad_pool_bn", &stem_wgrad_pool_bn,
        "ResNet stem maxpool + BN+ReLU backward fused into the stem weight gradient -> [dw, dgamma, dbeta]");
  m.def("stem_fwd", &stem_fwd,
        "{z, [P, 2, 64] partials}: ResNet 7x7/2 stem conv on MFMA with BN statistics (mv_stem.hip)",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("shift") = pybind11::none(),
        pybind11::arg("grid") = 0);
}
