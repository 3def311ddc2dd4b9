// PyTorch bindings for the mivod gfx950 kernels (module mivod._mvk).  The entry points
// live in one source per domain (mv_bind_optim / _bn / _bert / _gemm / _conv.cpp), each
// exporting a bind_<domain>(module).  Every entry point validates its operands on the host
// with the helpers of mv_checks.h before a launch: a kernel is never started on operands
// that disagree with the grid it assumes.  All launches go to the caller's current HIP
// stream.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>

#include <rocprofiler-sdk-roctx/roctx.h>

void bind_optim(pybind11::module_& m);
void bind_bn(pybind11::module_& m);
void bind_bert(pybind11::module_& m);
void bind_gemm(pybind11::module_& m);
void bind_conv(pybind11::module_& m);

// A tensor over device memory mivod owns elsewhere (the mesh's IPC staging
// slot): no copy, no deleter — the owner outlives every view by construction.
at::Tensor tensor_from_ptr(uintptr_t ptr, int64_t numel, at::ScalarType dtype, int64_t device) {
  TORCH_CHECK(ptr != 0 && numel >= 0, "tensor_from_ptr: bad pointer / size");
  TORCH_CHECK(ptr % 16 == 0, "tensor_from_ptr: pointer must be 16-byte aligned");
  return at::from_blob(reinterpret_cast<void*>(ptr), {numel},
                       at::TensorOptions().dtype(dtype).device(at::kCUDA, device));
}

PYBIND11_MODULE(_mvk, m) {
  m.doc() = "mivod hand-written gfx950 (CDNA4) kernels";
  m.def("tensor_from_ptr", &tensor_from_ptr, "tensor view of mivod-owned device memory");
  // roctx ranges: rocprofv3 --marker-trace shows mivod's bucket phases (pack,
  // allreduce, fused step) on the same timeline as the kernels and RCCL
  m.def("range_push", [](const std::string& s) { return roctxRangePushA(s.c_str()); });
  m.def("range_pop", []() { return roctxRangePop(); });
  m.def("mark", [](const std::string& s) { roctxMarkA(s.c_str()); });
  bind_optim(m);
  bind_bn(m);
  bind_bert(m);
  bind_gemm(m);
  bind_conv(m);
}
