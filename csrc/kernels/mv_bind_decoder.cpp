// mivod._mvk._decoder bindings: residual add + RMSNorm, SwiGLU, rotary position embedding on the
// grouped qkv layout (mv_decoder.h; the dw column sums finish in mv_bert.h's colsum kernel)
#include "mv_checks.h"
#include "mv_decoder.h"

namespace {
using namespace mvc;

// contiguous bf16 tensor of exactly M * N elements
void check_mn(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
              int64_t M, int64_t N) {
  check_nd(fn, what, t, like, -1);
  TORCH_CHECK(t.numel() == M * N, fn, ": ", what, " must hold ", M * N, " elements, not ",
              t.numel());
}

// the hidden size of a row kernel's operand [*, H] with weight [H] -> rows
int64_t rms_rows(const char* fn, const at::Tensor& x, const at::Tensor& w, int64_t* H) {
  check_nd(fn, "w", w, x, 1);
  *H = w.numel();
  TORCH_CHECK(*H >= 8 && *H % 8 == 0 && *H <= 8192, fn,
              ": hidden size must be a multiple of 8 in [8, 8192], not ", *H);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == *H, fn, ": last dim must equal the weight's ", *H);
  return x.numel() / *H;
}

// -> (y, v, rstd): v = res + z (z itself when res is None), rstd fp32 [M]
std::vector<at::Tensor> rms_fwd(at::Tensor z, OptTensor res, at::Tensor w, double eps) {
  const char* fn = "_decoder.rms_fwd";
  check_nd(fn, "z", z, z, -1);
  int64_t H;
  const int64_t M = rms_rows(fn, z, w, &H);
  if (given(res)) check_mn(fn, "res", *res, z, M, H);
  c10::DeviceGuard guard(z.device());
  at::Tensor y = at::empty_like(z);
  at::Tensor v = given(res) ? at::empty_like(z) : z;
  at::Tensor rstd = at::empty({M}, z.options().dtype(at::kFloat));
  if (M)
    mv_rms_fwd(z.data_ptr(), given(res) ? res->data_ptr() : nullptr, w.data_ptr(),
               given(res) ? v.data_ptr() : nullptr, y.data_ptr(), rstd.data_ptr<float>(), M, (int)H,
               (float)eps, cur_stream());
  return {y, v, rstd};
}

// -> (dv, dw).  dy None (y was not used): dv is dv_out itself and dw is zero, no launch.
std::vector<at::Tensor> rms_bwd(OptTensor dy, OptTensor dv_out, at::Tensor v, at::Tensor rstd,
                                at::Tensor w) {
  const char* fn = "_decoder.rms_bwd";
  check_nd(fn, "v", v, v, -1);
  int64_t H;
  const int64_t M = rms_rows(fn, v, w, &H);
  TORCH_CHECK(given(dy) || given(dv_out), fn, ": dy and dv_out cannot both be None");
  if (given(dy)) check_mn(fn, "dy", *dy, v, M, H);
  if (given(dv_out)) check_mn(fn, "dv_out", *dv_out, v, M, H);
  const float* rp = vec_ptr(fn, "rstd", rstd, v, M);
  c10::DeviceGuard guard(v.device());
  if (!given(dy) || M == 0) return {given(dy) ? at::empty_like(v) : *dv_out, at::zeros_like(w)};
  at::Tensor dv = at::empty_like(v), dw = at::empty_like(w);
  at::Tensor partial = at::empty({mv_rms_partials(M), H}, v.options().dtype(at::kFloat));
  mv_rms_bwd(dy->data_ptr(), given(dv_out) ? dv_out->data_ptr() : nullptr, v.data_ptr(), rp,
             w.data_ptr(), dv.data_ptr(), partial.data_ptr<float>(), dw.data_ptr(), M, (int)H,
             cur_stream());
  return {dv, dw};
}

// x [*, 2 N] -> rows; sets *N
int64_t swiglu_rows(const char* fn, const at::Tensor& x, int64_t* N) {
  check_nd(fn, "x", x, x, -1);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) >= 16 && x.size(-1) % 16 == 0, fn,
              ": x must be [*, 2 N] with N a positive multiple of 8");
  *N = x.size(-1) / 2;
  return x.numel() / (2 * *N);
}

at::Tensor swiglu_fwd(at::Tensor x) {
  const char* fn = "_decoder.swiglu_fwd";
  int64_t N;
  const int64_t M = swiglu_rows(fn, x, &N);
  c10::DeviceGuard guard(x.device());
  std::vector<int64_t> shape = x.sizes().vec();
  shape.back() = N;
  at::Tensor y = at::empty(shape, x.options());
  if (M) mv_swiglu_fwd(x.data_ptr(), y.data_ptr(), M, (int)N, cur_stream());
  return y;
}

at::Tensor swiglu_bwd(at::Tensor dy, at::Tensor x) {
  const char* fn = "_decoder.swiglu_bwd";
  int64_t N;
  const int64_t M = swiglu_rows(fn, x, &N);
  check_mn(fn, "dy", dy, x, M, N);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  if (M) mv_swiglu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), M, (int)N, cur_stream());
  return dx;
}

at::Tensor rotary(const char* fn, const at::Tensor& qkv, int64_t kv_heads, const at::Tensor& cos,
                  const at::Tensor& sin, const OptTensor& pos, bool adjoint) {
  check_nd(fn, "qkv", qkv, qkv, 4);
  TORCH_CHECK(qkv.size(3) == 128, fn, ": qkv must be [b, s, hq + 2 kv_heads, 128]");
  const int64_t b = qkv.size(0), s = qkv.size(1), heads = qkv.size(2);
  TORCH_CHECK(kv_heads >= 1 && heads > 2 * kv_heads && (heads - 2 * kv_heads) % kv_heads == 0, fn,
              ": qkv's ", heads, " heads must be hq + 2 kv_heads with hq a multiple of kv_heads = ",
              kv_heads);
  check_nd(fn, "cos", cos, qkv, 2, at::kFloat);
  check_nd(fn, "sin", sin, qkv, 2, at::kFloat);
  const int64_t P = cos.size(0);
  TORCH_CHECK(cos.size(1) == 64 && sin.size(1) == 64 && sin.size(0) == P && P >= 1, fn,
              ": cos and sin must be [P, 64] tables of one length");
  TORCH_CHECK(P < (int64_t(1) << 31) && heads < (int64_t(1) << 20) && s < (int64_t(1) << 31) &&
                  b * s * heads < (int64_t(1) << 35),
              fn, ": qkv or tables too large");
  const int32_t* pp = vec_ptr_opt<int32_t>(fn, "pos", pos, qkv, b * s);
  TORCH_CHECK(pp || s <= P, fn, ": ", s, " positions need tables of at least that many rows, not ",
              P, " (or pass pos)");
  c10::DeviceGuard guard(qkv.device());
  at::Tensor out = at::empty_like(qkv);
  if (qkv.numel())
    mv_rotary(qkv.data_ptr(), out.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pp,
              b * s, (int)s, (int)heads, (int)(heads - kv_heads), (int)P, adjoint, cur_stream());
  return out;
}

}  // namespace

void bind_decoder(pybind11::module_& m) {
  using Opt = c10::optional<at::Tensor>;
  // the top-level surface is a snapshot (tests/mvk_api.json): a private submodule
  pybind11::module_ d = m.def_submodule(
      "_decoder", "decoder-block kernels: residual add + RMSNorm, SwiGLU, rotary embedding");
  d.def("rms_fwd", &rms_fwd, "(z, res | None, w, eps) -> (y, v = res + z, rstd)",
        pybind11::arg("z"), pybind11::arg("res"), pybind11::arg("w"), pybind11::arg("eps"));
  d.def("rms_bwd", &rms_bwd, "(dy | None, dv_out | None, v, rstd, w) -> (dv, dw)",
        pybind11::arg("dy"), pybind11::arg("dv_out"), pybind11::arg("v"), pybind11::arg("rstd"),
        pybind11::arg("w"));
  d.def("swiglu_fwd", &swiglu_fwd, "x [*, 2 N] -> silu(x[:, :N]) x[:, N:]");
  d.def("swiglu_bwd", &swiglu_bwd, "(dy, x) -> dx");
  d.def("rotary_fwd",
        [](at::Tensor qkv, int64_t kv_heads, at::Tensor cos, at::Tensor sin, Opt pos) {
          return rotary("_decoder.rotary_fwd", qkv, kv_heads, cos, sin, pos, false);
        },
        "rotate the query and key heads of qkv [b, s, hq + 2 kv_heads, 128]; value heads copied",
        pybind11::arg("qkv"), pybind11::arg("kv_heads"), pybind11::arg("cos"), pybind11::arg("sin"),
        pybind11::arg("pos") = pybind11::none());
  d.def("rotary_bwd",
        [](at::Tensor dout, int64_t kv_heads, at::Tensor cos, at::Tensor sin, Opt pos) {
          return rotary("_decoder.rotary_bwd", dout, kv_heads, cos, sin, pos, true);
        },
        "the adjoint of rotary_fwd on the gradient of its output", pybind11::arg("dout"),
        pybind11::arg("kv_heads"), pybind11::arg("cos"), pybind11::arg("sin"),
        pybind11::arg("pos") = pybind11::none());
}
