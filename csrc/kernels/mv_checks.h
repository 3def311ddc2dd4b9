// Operand checks shared by the binding sources (mv_bind_*.cpp) of mivod._mvk.
// Every helper takes the binding's exported name, the operand's name and the
// tensor whose device the operand must share (the primary operand, which may be
// the operand itself), and checks four things: GPU, dtype, layout, same device.
// A failure reads "<binding>: <operand> must be ...".  TORCH_CHECK formats its
// message only on failure: the success path allocates nothing.
// (ATen + torch's pybind casters, not torch/extension.h: the C++ frontend it pulls in
// doubles the compile time of every binding source.)
#pragma once
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <torch/csrc/utils/pybind.h>

#include <vector>

namespace mvc {

using OptTensor = c10::optional<at::Tensor>;

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

inline int dtype_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default: TORCH_CHECK(false, "mivod kernels: unsupported dtype ", t.scalar_type());
  }
  return -1;
}

inline bool given(const OptTensor& t) { return t.has_value() && t->defined(); }

inline void check_device(const char* fn, const char* what, const at::Tensor& t,
                         const at::Tensor& like) {
  TORCH_CHECK(t.device() == like.device(), fn, ": ", what, " must be on ", like.device(),
              " like the primary operand, not ", t.device());
}

// GPU + dtype + device, any layout: the part every helper below starts with
inline void check_on(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
                     at::ScalarType dt) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt, fn, ": ", what, " must be a ", dt,
              " GPU tensor");
  check_device(fn, what, t, like);
}

// contiguous tensor of `dt` with `ndim` dimensions (ndim < 0: any)
inline void check_nd(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
                     int64_t ndim, at::ScalarType dt = at::kBFloat16) {
  check_on(fn, what, t, like, dt);
  TORCH_CHECK(t.is_contiguous(), fn, ": ", what, " must be contiguous");
  TORCH_CHECK(ndim < 0 || t.dim() == ndim, fn, ": ", what, " must be ", ndim, "-D");
}

// channels_last 4-D bf16 activation / filter whose channel count is a multiple of cmult
inline void check_chlast(const char* fn, const char* what, const at::Tensor& t,
                         const at::Tensor& like, int64_t cmult = 1) {
  check_on(fn, what, t, like, at::kBFloat16);
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  t.size(1) % cmult == 0,
              fn, ": ", what, " must be channels_last 4-D with C % ", cmult, " == 0");
}

// the BN family's activation: channels_last 4-D or contiguous 2-D bf16, C % 8 == 0;
// returns the rows and sets *C
inline int64_t check_act(const char* fn, const char* what, const at::Tensor& t,
                         const at::Tensor& like, int64_t* C) {
  check_on(fn, what, t, like, at::kBFloat16);
  TORCH_CHECK((t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast)) ||
                  (t.dim() == 2 && t.is_contiguous()),
              fn, ": ", what, " must be channels_last 4-D or contiguous 2-D");
  *C = t.size(1);
  TORCH_CHECK(*C > 0 && *C % 8 == 0, fn, ": ", what,
              " must have a channel count that is a multiple of 8");
  return t.numel() / *C;
}

// contiguous tensor of `dt` holding exactly n (at_least: >= n) elements -> its pointer
template <typename T = float>
inline T* vec_ptr(const char* fn, const char* what, const at::Tensor& t, const at::Tensor& like,
                  int64_t n, bool at_least = false) {
  check_nd(fn, what, t, like, -1, c10::CppTypeToScalarType<T>::value);
  TORCH_CHECK(at_least ? t.numel() >= n : t.numel() == n, fn, ": ", what, " must hold ",
              at_least ? "at least " : "exactly ", n, " elements, not ", t.numel());
  return t.data_ptr<T>();
}

// the same for an optional operand: nullptr when it is None
template <typename T = float>
inline T* vec_ptr_opt(const char* fn, const char* what, const OptTensor& t, const at::Tensor& like,
                      int64_t n, bool at_least = false) {
  return given(t) ? vec_ptr<T>(fn, what, *t, like, n, at_least) : nullptr;
}

// flat dense buffer of a kernel dtype (fp32 / bf16 / fp16); contiguous unless told otherwise
inline void check_dense(const char* fn, const char* what, const at::Tensor& t,
                        const at::Tensor& like, bool contiguous = true) {
  const at::ScalarType dt = t.scalar_type();
  TORCH_CHECK(t.is_cuda() && (dt == at::kFloat || dt == at::kBFloat16 || dt == at::kHalf), fn, ": ",
              what, " must be a fp32 / bf16 / fp16 GPU tensor");
  check_device(fn, what, t, like);
  TORCH_CHECK(contiguous ? t.is_contiguous() : t.is_non_overlapping_and_dense(), fn, ": ", what,
              " must be ", contiguous ? "contiguous" : "dense and non-overlapping");
}

}  // namespace mvc
