// mivod._mvk bindings: implicit-GEMM 3x3 / 1x1 convolutions (pad 1 / 0), their data and
// weight gradients and the data-gradient filter transpose, channels_last bf16 (mv_conv.h)
#include "mv_checks.h"
#include "mv_conv.h"

namespace {
using namespace mvc;

int64_t conv3x3_partials(int64_t M, int64_t K) { return mv_conv3x3_partials(M, (int)K); }

// y = conv3x3(x, w, stride, pad 1) / conv1x1(x, w, stride) (+ BN statistics partials of y
// around shift).  in_scale, in_bias (3x3 only): x is the producing BN's input;
// relu(x * in_scale + in_bias) is convolved without being materialised — the 64 -> 64
// stride-1 row-patch kernel only.
at::Tensor conv_nhwc(const char* fn, int64_t ks, const at::Tensor& x, const at::Tensor& w,
                     int64_t stride, const OptTensor& shift, const OptTensor& partial,
                     const OptTensor& in_scale, const OptTensor& in_bias) {
  check_chlast(fn, "x", x, x, 64);
  check_chlast(fn, "w", w, x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3), K = w.size(0);
  TORCH_CHECK(w.size(1) == C && w.size(2) == ks && w.size(3) == ks, fn,
              ": w must be a [K, C, ", ks, ", ", ks, "] filter matching x");
  TORCH_CHECK(K % 64 == 0 && C > 0 && K > 0, fn, ": C and K must be multiples of 64");
  TORCH_CHECK(stride == 1 || stride == 2, fn, ": stride must be 1 or 2");
  TORCH_CHECK(N * H * W * std::max(C, K) < (int64_t(1) << 40) && H < 65536 && W < 65536, fn,
              ": too large");
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t M = N * Ho * Wo;
  TORCH_CHECK(M > 0, fn, ": empty input");
  float* pp = vec_ptr_opt(fn, "partial", partial, x, conv3x3_partials(M, K) * 2 * K, true);
  const float* sp = pp ? vec_ptr_opt(fn, "shift", shift, x, K) : nullptr;
  const float* isc = vec_ptr_opt(fn, "in_scale", in_scale, x, C);
  const float* ibi = vec_ptr_opt(fn, "in_bias", in_bias, x, C);
  TORCH_CHECK((isc == nullptr) == (ibi == nullptr), fn, ": in_scale and in_bias go together");
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty({N, K, Ho, Wo}, x.options(), at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(mv_conv_nhwc(x.data_ptr(), w.data_ptr(), y.data_ptr(), (int)N, (int)H, (int)W,
                           (int)C, (int)K, (int)ks, (int)stride, sp, pp, cur_stream(), nullptr,
                           nullptr, isc, ibi),
              fn, ": unsupported shape");
  return y;
}

// data gradient of a stride-1 3x3 conv (dy . flipped filter) with the mode-1 (BN+ReLU)
// backward reduce of the BN that produced the conv's input fused into the epilogue:
// returns (d = relu'(x_bn) * dgrad, partials [P, 2, C]).  Also the stride-1 1x1 conv
// (wt [C, K, 1, 1]): the same kernel with ks = 1.
std::vector<at::Tensor> conv3x3_bn_bwd(at::Tensor dy, at::Tensor wt, at::Tensor x_bn,
                                       at::Tensor vec) {
  const char* fn = "conv3x3_bn_bwd";
  check_chlast(fn, "dy", dy, dy, 64);
  check_chlast(fn, "wt", wt, dy, 64);
  const int64_t N = dy.size(0), K = dy.size(1), H = dy.size(2), W = dy.size(3), C = wt.size(0);
  TORCH_CHECK(wt.size(1) == K && wt.size(2) == wt.size(3) && (wt.size(2) == 3 || wt.size(2) == 1) &&
                  C % 64 == 0,
              "conv3x3_bn_bwd: wt must be the [C, K, ks, ks] (ks 3 or 1) transposed filter with "
              "C % 64 == 0");
  check_chlast(fn, "x_bn", x_bn, dy);
  TORCH_CHECK(x_bn.sizes() == at::IntArrayRef({N, C, H, W}),
              "conv3x3_bn_bwd: x_bn must be the BN input [N, C, H, W]");
  const float* vp = vec_ptr(fn, "vec", vec, dy, 4 * C);
  TORCH_CHECK(N * H * W * std::max(C, K) < (int64_t(1) << 40) && H < 65536 && W < 65536,
              "conv3x3_bn_bwd: too large");
  c10::DeviceGuard guard(dy.device());
  const int64_t M = N * H * W;
  at::Tensor d = at::empty({N, C, H, W}, dy.options(), at::MemoryFormat::ChannelsLast);
  at::Tensor part = at::empty({conv3x3_partials(M, C), 2, C}, dy.options().dtype(at::kFloat));
  TORCH_CHECK(mv_conv_nhwc(dy.data_ptr(), wt.data_ptr(), d.data_ptr(), (int)N, (int)H, (int)W,
                           (int)K, (int)C, (int)wt.size(2), 1, nullptr, part.data_ptr<float>(),
                           cur_stream(), x_bn.data_ptr(), vp),
              "conv3x3_bn_bwd: unsupported shape");
  return {d, part};
}

// data gradient of a stride-2 3x3 conv (pad 1) as four output-parity-class gather GEMMs
// (mv_conv.hip / mv_gemm256.hip): dy [N, K, H/2, W/2], wt the transposed flipped filter
// [C, K, 3, 3] -> dx [N, C, H, W].  Returns [] when the shape is not covered (the caller
// falls back).
std::vector<at::Tensor> conv3x3_s2_dgrad(at::Tensor dy, at::Tensor wt, int64_t H, int64_t W) {
  check_chlast("conv3x3_s2_dgrad", "dy", dy, dy);
  check_chlast("conv3x3_s2_dgrad", "wt", wt, dy);
  TORCH_CHECK(wt.size(2) == 3 && wt.size(3) == 3 && wt.size(1) == dy.size(1),
              "conv3x3_s2_dgrad: wt must be the [C, K, 3, 3] transposed filter");
  const int64_t N = dy.size(0), K = dy.size(1), C = wt.size(0);
  TORCH_CHECK(H > 0 && W > 0 && (H - 1) / 2 + 1 == dy.size(2) && (W - 1) / 2 + 1 == dy.size(3),
              "conv3x3_s2_dgrad: H, W do not match dy");
  if (H >= 65536 || W >= 65536 || N >= (int64_t(1) << 31) ||
      !mv_conv3x3_s2_dgrad_supported((int)N, (int)H, (int)W, (int)C, (int)K))
    return {};
  c10::DeviceGuard guard(dy.device());
  at::Tensor dx = at::empty({N, C, H, W}, dy.options(), at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(mv_conv3x3_s2_dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), (int)N, (int)H,
                                  (int)W, (int)C, (int)K, cur_stream()),
              "conv3x3_s2_dgrad: launch refused");
  return {dx};
}

// Data-gradient filters of many convs in one launch: for every channels_last bf16 w
// [K, C, ks, ks] the channels_last [C, K, ks, ks] filter with the taps rotated 180 degrees
// (w.transpose(0, 1).flip(2, 3); for 1x1 W^T).  Outputs and the device block table are
// cached per input set (the filters live in the optimizer's arena: stable pointers), so a
// step costs one kernel.
std::vector<at::Tensor> transpose_filters(std::vector<at::Tensor> ws) {
  struct Entry {
    std::vector<const void*> src;
    std::vector<at::Tensor> outs;
    at::Tensor table;
    int64_t blocks = 0;
  };
  // (heap-allocated and never destroyed: tensors must not be freed after the HIP runtime at
  // process exit)
  static std::vector<Entry>& cache = *new std::vector<Entry>();
  TORCH_CHECK(!ws.empty(), "transpose_filters: no filters");
  const int n = (int)ws.size();
  std::vector<const void*> src(n);
  std::vector<int> K(n), C(n), ks(n);
  for (int i = 0; i < n; ++i) {
    const at::Tensor& w = ws[i];
    check_chlast("transpose_filters", "ws", w, ws[0]);
    TORCH_CHECK(w.size(2) == w.size(3), "transpose_filters: ws must be [K, C, k, k] filters");
    src[i] = w.data_ptr();
    K[i] = (int)w.size(0);
    C[i] = (int)w.size(1);
    ks[i] = (int)w.size(2);
  }
  c10::DeviceGuard guard(ws[0].device());
  Entry* e = nullptr;
  for (auto& c : cache) {
    if (c.src != src || (int)c.outs.size() != n) continue;
    bool same = true;
    for (int i = 0; i < n && same; ++i)
      same = c.outs[i].size(0) == C[i] && c.outs[i].size(1) == K[i] && c.outs[i].size(2) == ks[i] &&
             c.outs[i].device() == ws[i].device();
    if (same) { e = &c; break; }
  }
  if (!e) {
    if (cache.size() >= 8) cache.erase(cache.begin());
    Entry ne;
    ne.src = src;
    std::vector<void*> dst(n);
    for (int i = 0; i < n; ++i) {
      ne.outs.push_back(at::empty({C[i], K[i], ks[i], ks[i]}, ws[i].options(),
                                  at::MemoryFormat::ChannelsLast));
      dst[i] = ne.outs[i].data_ptr();
    }
    ne.blocks = mv_transpose_filters_blocks(K.data(), C.data(), ks.data(), n);
    const int64_t bytes = mv_transpose_filters_table_bytes(n, ne.blocks);
    at::Tensor host = at::empty({bytes}, at::TensorOptions().dtype(at::kByte).pinned_memory(true));
    mv_transpose_filters_table(src.data(), dst.data(), K.data(), C.data(), ks.data(), n,
                               host.data_ptr());
    ne.table = host.to(ws[0].device(), /*non_blocking=*/false);
    cache.push_back(std::move(ne));
    e = &cache.back();
  }
  mv_transpose_filters(e->table.data_ptr(), n, e->blocks, cur_stream());
  return e->outs;
}

// x, dy of y = conv(x, w, stride) for a weight gradient: sets the extents, returns M
int64_t check_wgrad(const char* fn, const at::Tensor& x, const at::Tensor& dy, int64_t stride,
                    int64_t* Ho, int64_t* Wo) {
  check_chlast(fn, "x", x, x, 64);
  check_chlast(fn, "dy", dy, x);
  TORCH_CHECK(stride == 1 || stride == 2, fn, ": stride must be 1 or 2");
  *Ho = (x.size(2) - 1) / stride + 1;
  *Wo = (x.size(3) - 1) / stride + 1;
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(2) == *Ho && dy.size(3) == *Wo, fn,
              ": dy shape");
  return x.size(0) * *Ho * *Wo;
}

// weight gradient of y = conv3x3(x, w, stride, pad 1): dw [K, C, 3, 3] channels_last bf16
at::Tensor wgrad3x3(at::Tensor x, at::Tensor dy, int64_t stride,
                    c10::optional<at::Tensor> in_scale, c10::optional<at::Tensor> in_bias) {
  int64_t Ho, Wo;
  const int64_t M = check_wgrad("wgrad3x3", x, dy, stride, &Ho, &Wo);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3), K = dy.size(1);
  TORCH_CHECK(K % 64 == 0 && N * H * W * std::max(C, K) < (int64_t(1) << 40),
              "wgrad3x3: channels must be multiples of 64");
  const float* isc = vec_ptr_opt("wgrad3x3", "in_scale", in_scale, x, C);
  const float* ibi = vec_ptr_opt("wgrad3x3", "in_bias", in_bias, x, C);
  TORCH_CHECK((isc == nullptr) == (ibi == nullptr), "wgrad3x3: in_scale and in_bias go together");
  c10::DeviceGuard guard(x.device());
  at::Tensor work = at::empty({mv_wgrad3x3_workspace(M, (int)K, (int)C)},
                              x.options().dtype(at::kFloat));
  at::Tensor dw = at::empty({K, C, 3, 3}, x.options(), at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(mv_wgrad3x3(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), work.data_ptr<float>(),
                          (int)N, (int)H, (int)W, (int)C, (int)K, (int)stride, cur_stream(), isc,
                          ibi),
              "wgrad3x3: unsupported shape");
  return dw;
}

// weight gradient of y = conv1x1(x, w, stride, pad 0): dw [K, C, 1, 1] bf16
at::Tensor wgrad1x1(at::Tensor x, at::Tensor dy, int64_t stride, bool fp32_out,
                    c10::optional<at::Tensor> dy2) {
  int64_t Ho, Wo;
  const int64_t M = check_wgrad("wgrad1x1", x, dy, stride, &Ho, &Wo);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3), K1 = dy.size(1);
  // dy2: a second dy stream stacked below dy's channels (dw = [dy | dy2]^T . x)
  const bool two = given(dy2);
  int64_t K = K1;
  bool gather = false;
  if (two) {
    // [N, K2, Ho, Wo] at the output rows, or (stride 2) [N, K2, H, W] read at each output
    // row's strided input pixel (e.g. dy2 = x itself: the Gram pass of x[:, :, ::2, ::2])
    check_chlast("wgrad1x1", "dy2", *dy2, x, 64);
    gather = stride > 1 && dy2->size(2) == H && dy2->size(3) == W;
    TORCH_CHECK(dy2->size(0) == N && (gather || (dy2->size(2) == Ho && dy2->size(3) == Wo)),
                "wgrad1x1: dy2 must be [N, K2, Ho, Wo] (or, stride 2, [N, K2, H, W])");
    K = K1 + dy2->size(1);
  }
  TORCH_CHECK(K % 64 == 0 && N * H * W * std::max(C, K) < (int64_t(1) << 40),
              "wgrad1x1: channels must be multiples of 64");
  c10::DeviceGuard guard(x.device());
  at::Tensor work = at::empty({mv_wgrad1x1_workspace(M, (int)K, (int)C)},
                              x.options().dtype(at::kFloat));
  at::Tensor dw = at::empty({K, C, 1, 1}, fp32_out ? x.options().dtype(at::kFloat) : x.options(),
                            at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(mv_wgrad1x1(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), work.data_ptr<float>(),
                          (int)N, (int)H, (int)W, (int)C, (int)K, (int)stride, cur_stream(),
                          fp32_out, two ? dy2->data_ptr() : nullptr, (int)K1, gather),
              "wgrad1x1: unsupported shape");
  return dw;
}

}  // namespace

void bind_conv(pybind11::module_& m) {
  namespace py = pybind11;
  using Opt = c10::optional<at::Tensor>;
  m.def("conv3x3",
        [](at::Tensor x, at::Tensor w, int64_t stride, Opt shift, Opt partial, Opt in_scale,
           Opt in_bias) {
          return conv_nhwc("conv3x3", 3, x, w, stride, shift, partial, in_scale, in_bias);
        },
        "implicit-GEMM 3x3 conv (pad 1) with optional fused BN statistics "
        "(in_scale / in_bias: x is the producing BN's input, its BN + ReLU applied on load)",
        py::arg("x"), py::arg("w"), py::arg("stride") = 1, py::arg("shift") = py::none(),
        py::arg("partial") = py::none(), py::arg("in_scale") = py::none(),
        py::arg("in_bias") = py::none());
  m.def("conv1x1",
        [](at::Tensor x, at::Tensor w, int64_t stride, Opt shift, Opt partial) {
          return conv_nhwc("conv1x1", 1, x, w, stride, shift, partial, c10::nullopt, c10::nullopt);
        },
        "1x1 conv (implicit-GEMM kernel) with optional fused BN statistics",
        py::arg("x"), py::arg("w"), py::arg("stride") = 1, py::arg("shift") = py::none(),
        py::arg("partial") = py::none());
  m.def("conv3x3_bn_bwd", &conv3x3_bn_bwd,
        "stride-1 3x3 data gradient with the producing BN+ReLU's backward reduce fused");
  m.def("conv3x3_s2_dgrad", &conv3x3_s2_dgrad,
        "stride-2 3x3 data gradient (parity-class gather GEMMs); [] when the shape is not "
        "covered", py::arg("dy"), py::arg("wt"), py::arg("H"), py::arg("W"));
  m.def("wgrad1x1", &wgrad1x1, "1x1 (pad 0, stride 1/2) conv weight gradient on MFMA",
        py::arg("x"), py::arg("dy"), py::arg("stride") = 1, py::arg("fp32_out") = false,
        py::arg("dy2") = py::none());
  m.def("transpose_filters", &transpose_filters,
        "data-gradient filters (transposed, taps rotated) of many convs in one launch");
  m.def("wgrad3x3", &wgrad3x3, "3x3 (pad 1) conv weight gradient on MFMA (transposed LDS reads)",
        py::arg("x"), py::arg("dy"), py::arg("stride") = 1, py::arg("in_scale") = py::none(),
        py::arg("in_bias") = py::none());
  m.def("conv3x3_partials", &conv3x3_partials, "partial rows of conv3x3's statistics epilogue");
}
