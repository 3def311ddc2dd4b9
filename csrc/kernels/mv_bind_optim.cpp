// mivod._mvk bindings: multi-tensor pack / cast, fused optimizer steps, global gradient-norm
// clipping, local gradient accumulation, weight averaging, Adasum (mv_kernels.h, mv_adaptive.h,
// mv_adamfam.h, mv_clip.h, mv_accum.h, mv_ema.h)
#include "mv_accum.h"
#include "mv_adamfam.h"
#include "mv_adaptive.h"
#include "mv_checks.h"
#include "mv_clip.h"
#include "mv_ema.h"
#include "mv_kernels.h"

#include <algorithm>

namespace {
using namespace mvc;

constexpr int64_t kChunk = 4096;

// optional int32 device flag (non-finite result / fp16-wire overflow skip)
int* flag_ptr(const char* fn, const char* what, const OptTensor& f, const at::Tensor& like) {
  return vec_ptr_opt<int>(fn, what, f, like, 1, true);
}

// The tensor table of a multi-tensor launch: checks every tensor (dense, one dtype, on
// `flat`'s device, [offsets[i], +numel) inside fnumel elements) and calls launch(table) once
// per kMvMaxTensors tensors / 2^30 chunks.
template <typename Launch>
void mt_tables(const char* fn, const std::vector<at::Tensor>& tensors, const at::Tensor& flat,
               const std::vector<int64_t>& offsets, int64_t fnumel, Launch launch) {
  const int tdt = dtype_code(tensors[0]);
  MtArgs a;
  a.ntensors = 0;
  a.chunk_start[0] = 0;
  auto flush = [&]() {
    if (a.ntensors == 0) return;
    launch(a);
    a.ntensors = 0;
    a.chunk_start[0] = 0;
  };
  for (size_t i = 0; i < tensors.size(); ++i) {
    const at::Tensor& t = tensors[i];
    check_dense(fn, "tensors", t, flat, false);
    TORCH_CHECK(dtype_code(t) == tdt, fn, ": mixed tensor dtypes in one call");
    const int64_t n = t.numel();
    TORCH_CHECK(offsets[i] >= 0 && offsets[i] + n <= fnumel, fn, ": tensor ", i,
                " [", offsets[i], ", +", n, ") exceeds flat buffer of ", fnumel);
    if (n == 0) continue;
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    TORCH_CHECK(chunks < (1 << 30), fn, ": tensor too large");
    if (a.ntensors == kMvMaxTensors ||
        (int64_t)a.chunk_start[a.ntensors] + chunks > (int64_t)(1u << 30))
      flush();
    const int k = a.ntensors++;
    a.ptr[k] = t.data_ptr();
    a.numel[k] = n;
    a.flat_off[k] = offsets[i];
    a.chunk_start[k + 1] = a.chunk_start[k] + (int32_t)chunks;
  }
  flush();
}

// K1/K2: pack (to_flat) or unpack tensors <-> flat[offsets[i] : offsets[i]+numel]
void mt_copy(const std::vector<at::Tensor>& tensors, at::Tensor flat,
             const std::vector<int64_t>& offsets, bool to_flat, double scale,
             c10::optional<at::Tensor> nonfinite) {
  TORCH_CHECK(tensors.size() == offsets.size(), "mt_copy: tensors/offsets length mismatch");
  if (tensors.empty()) return;
  check_dense("mt_copy", "tensors", tensors[0], tensors[0], false);
  check_dense("mt_copy", "flat", flat, tensors[0]);
  c10::DeviceGuard guard(flat.device());
  const int tdt = dtype_code(tensors[0]);
  const int fdt = dtype_code(flat);
  int* nf = flag_ptr("mt_copy", "nonfinite", nonfinite, flat);
  hipStream_t st = cur_stream();
  mt_tables("mt_copy", tensors, flat, offsets, flat.numel(), [&](const MtArgs& a) {
    mv_launch_mt_copy(a, tdt, flat.data_ptr(), fdt, to_flat, (float)scale, nf, st);
  });
}

// Local gradient accumulation (mv_accum.hip): acc[offsets[i] : +numel] = (first) or += float(t_i)
void accumulate(const std::vector<at::Tensor>& tensors, at::Tensor acc,
                const std::vector<int64_t>& offsets, bool first) {
  TORCH_CHECK(tensors.size() == offsets.size(), "accumulate: tensors/offsets length mismatch");
  if (tensors.empty()) return;
  check_dense("accumulate", "tensors", tensors[0], tensors[0], false);
  float* ap = vec_ptr("accumulate", "acc", acc, tensors[0], 0, true);
  c10::DeviceGuard guard(acc.device());
  const int tdt = dtype_code(tensors[0]);
  hipStream_t st = cur_stream();
  mt_tables("accumulate", tensors, acc, offsets, acc.numel(), [&](const MtArgs& a) {
    mv_launch_accumulate(a, tdt, ap, first, st);
  });
}

// dst[offsets[i] : +numel] = cast((acc[offsets[i] : +numel] + float(t_i)) * scale); acc is read
void pack_accumulated(const std::vector<at::Tensor>& tensors, at::Tensor acc, at::Tensor dst,
                      const std::vector<int64_t>& offsets, double scale,
                      c10::optional<at::Tensor> nonfinite) {
  TORCH_CHECK(tensors.size() == offsets.size(),
              "pack_accumulated: tensors/offsets length mismatch");
  if (tensors.empty()) return;
  check_dense("pack_accumulated", "tensors", tensors[0], tensors[0], false);
  check_dense("pack_accumulated", "dst", dst, tensors[0]);
  const float* ap = vec_ptr("pack_accumulated", "acc", acc, tensors[0], 0, true);
  c10::DeviceGuard guard(dst.device());
  const int tdt = dtype_code(tensors[0]);
  const int wdt = dtype_code(dst);
  int* nf = flag_ptr("pack_accumulated", "nonfinite", nonfinite, dst);
  hipStream_t st = cur_stream();
  // every range must lie inside both flat buffers
  const int64_t fnumel = std::min(acc.numel(), dst.numel());
  mt_tables("pack_accumulated", tensors, dst, offsets, fnumel, [&](const MtArgs& a) {
    mv_launch_pack_accumulated(a, tdt, ap, dst.data_ptr(), wdt, (float)scale, nf, st);
  });
}

void flat_cast(at::Tensor src, at::Tensor dst, double scale, c10::optional<at::Tensor> nonfinite) {
  check_dense("flat_cast", "src", src, src);
  check_dense("flat_cast", "dst", dst, src);
  TORCH_CHECK(src.numel() == dst.numel(), "flat_cast: numel mismatch");
  c10::DeviceGuard guard(src.device());
  mv_launch_flat_cast(src.data_ptr(), dtype_code(src), dst.data_ptr(), dtype_code(dst), src.numel(),
                      (float)scale, flag_ptr("flat_cast", "nonfinite", nonfinite, src),
                      cur_stream());
}

void nonfinite_scan(at::Tensor x, at::Tensor flag) {
  check_dense("nonfinite_scan", "x", x, x);
  int* fp = vec_ptr<int>("nonfinite_scan", "flag", flag, x, 1, true);
  c10::DeviceGuard guard(x.device());
  mv_launch_nonfinite_scan(x.data_ptr(), dtype_code(x), x.numel(), fp, cur_stream());
}

// sgd_step / adam_step / adadelta_step refuse an operand that is not 16-byte aligned.  Their
// kernels (on mv_flat_step.h's skeleton, which guards its vector body) would take an offset
// view, but the binding keeps refusing one: the arenas hand all three 64-element-aligned
// slices, that is their contract and the existing behaviour.  LARS, LAMB, RMSprop, Adagrad and
// the mivod._mvk._adamfam steps take any offset.
void check_aligned16(const char* fn, const char* what, const void* p) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, fn, ": ", what,
              " must be 16-byte aligned");
}

// The operands every fused step shares: the flat gradient, the fp32 master weights, the
// optional low-precision model copy, the device hyperparameter block [lr, first, bc1, bc2]
// (HIP-graph replays), the skip flag and the clip coefficient (given only through the
// mivod._mvk._clip entry points; the public ones pass none).
struct StepArgs {
  float* w;
  void* model = nullptr;
  int model_dt = 0;
  const float* dyn;
  const int* skip;
  const float* gclip;
};

const OptTensor kNoClip;

StepArgs step_args(const char* fn, const at::Tensor& g, const at::Tensor& w, const OptTensor& model,
                   const OptTensor& dyn, const OptTensor& skip, const OptTensor& gclip,
                   bool aligned = true) {
  check_dense(fn, "grad", g, g);
  if (aligned) check_aligned16(fn, "grad", g.data_ptr());
  StepArgs s;
  s.w = vec_ptr(fn, "master", w, g, g.numel());
  if (aligned) check_aligned16(fn, "master", s.w);
  if (given(model)) {
    check_dense(fn, "model", *model, g);
    TORCH_CHECK(model->numel() == g.numel(), fn, ": model numel mismatch");
    s.model = model->data_ptr();
    if (aligned) check_aligned16(fn, "model", s.model);
    s.model_dt = dtype_code(*model);
  }
  s.dyn = vec_ptr_opt(fn, "dyn", dyn, g, 4, true);
  s.skip = flag_ptr(fn, "skip", skip, g);
  s.gclip = vec_ptr_opt(fn, "gclip", gclip, g, 1, true);
  return s;
}

void sgd_impl(const at::Tensor& g, const at::Tensor& w, const OptTensor& mom,
              const OptTensor& model, double lr, double momentum, double dampening, double wd,
              double gscale, bool nesterov, bool first, const OptTensor& dyn,
              const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("sgd_step", g, w, model, dyn, skip, gclip);
  float* mp = vec_ptr_opt("sgd_step", "momentum", mom, g, g.numel());
  check_aligned16("sgd_step", "momentum", mp);
  c10::DeviceGuard guard(g.device());
  mv_launch_sgd(g.data_ptr(), dtype_code(g), s.w, mp, s.model, s.model_dt, g.numel(), (float)lr,
                (float)momentum, dampening, (float)wd, (float)gscale, nesterov, first,
                s.dyn, s.skip, s.gclip, cur_stream());
}

void sgd_step(at::Tensor g, at::Tensor w, c10::optional<at::Tensor> mom,
              c10::optional<at::Tensor> model, double lr, double momentum, double dampening,
              double wd, double gscale, bool nesterov, bool first, c10::optional<at::Tensor> dyn,
              c10::optional<at::Tensor> skip) {
  sgd_impl(g, w, mom, model, lr, momentum, dampening, wd, gscale, nesterov, first, dyn, skip,
           kNoClip);
}

void sgd_step_clip(at::Tensor g, at::Tensor w, c10::optional<at::Tensor> mom,
                   c10::optional<at::Tensor> model, double lr, double momentum, double dampening,
                   double wd, double gscale, bool nesterov, bool first,
                   c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                   at::Tensor gclip) {
  sgd_impl(g, w, mom, model, lr, momentum, dampening, wd, gscale, nesterov, first, dyn, skip,
           gclip);
}

void adam_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& m, const at::Tensor& v,
               const OptTensor& model, double lr, double b1, double b2, double eps, double wd,
               double gscale, int64_t step, bool adamw, bool keras_eps, const OptTensor& dyn,
               const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("adam_step", g, w, model, dyn, skip, gclip);
  float* mp = vec_ptr("adam_step", "exp_avg", m, g, g.numel());
  float* vp = vec_ptr("adam_step", "exp_avg_sq", v, g, g.numel());
  check_aligned16("adam_step", "exp_avg", mp);
  check_aligned16("adam_step", "exp_avg_sq", vp);
  TORCH_CHECK(step >= 1, "adam_step: step must be >= 1");
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  c10::DeviceGuard guard(g.device());
  mv_launch_adam(g.data_ptr(), dtype_code(g), s.w, mp, vp, s.model, s.model_dt, g.numel(),
                 (float)lr, b1, b2, (float)eps, (float)wd, (float)gscale, (float)bc1,
                 (float)bc2, adamw, keras_eps, s.dyn, s.skip, s.gclip, cur_stream());
}

void adam_step(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v,
               c10::optional<at::Tensor> model, double lr, double b1, double b2, double eps,
               double wd, double gscale, int64_t step, bool adamw, bool keras_eps,
               c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip) {
  adam_impl(g, w, m, v, model, lr, b1, b2, eps, wd, gscale, step, adamw, keras_eps, dyn, skip,
            kNoClip);
}

void adam_step_clip(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v,
                    c10::optional<at::Tensor> model, double lr, double b1, double b2, double eps,
                    double wd, double gscale, int64_t step, bool adamw, bool keras_eps,
                    c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                    at::Tensor gclip) {
  adam_impl(g, w, m, v, model, lr, b1, b2, eps, wd, gscale, step, adamw, keras_eps, dyn, skip,
            gclip);
}

void adadelta_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& sq,
                   const at::Tensor& acc, const OptTensor& model, double lr, double rho, double eps,
                   double wd, double gscale, const OptTensor& dyn, const OptTensor& skip,
                   const OptTensor& gclip) {
  const StepArgs s = step_args("adadelta_step", g, w, model, dyn, skip, gclip);
  float* sp = vec_ptr("adadelta_step", "square_avg", sq, g, g.numel());
  float* ap = vec_ptr("adadelta_step", "acc_delta", acc, g, g.numel());
  check_aligned16("adadelta_step", "square_avg", sp);
  check_aligned16("adadelta_step", "acc_delta", ap);
  c10::DeviceGuard guard(g.device());
  mv_launch_adadelta(g.data_ptr(), dtype_code(g), s.w, sp, ap, s.model, s.model_dt, g.numel(),
                     (float)lr, rho, (float)eps, (float)wd, (float)gscale, s.dyn, s.skip,
                     s.gclip, cur_stream());
}

void adadelta_step(at::Tensor g, at::Tensor w, at::Tensor sq, at::Tensor acc,
                   c10::optional<at::Tensor> model, double lr, double rho, double eps, double wd,
                   double gscale, c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip) {
  adadelta_impl(g, w, sq, acc, model, lr, rho, eps, wd, gscale, dyn, skip, kNoClip);
}

void adadelta_step_clip(at::Tensor g, at::Tensor w, at::Tensor sq, at::Tensor acc,
                        c10::optional<at::Tensor> model, double lr, double rho, double eps,
                        double wd, double gscale, c10::optional<at::Tensor> dyn,
                        c10::optional<at::Tensor> skip, at::Tensor gclip) {
  adadelta_impl(g, w, sq, acc, model, lr, rho, eps, wd, gscale, dyn, skip, gclip);
}

// the chunk -> segment tables of the segmented kernels, on `like`'s device
ChunkTable make_table(const char* fn, const at::Tensor& like, const at::Tensor& begin,
                      const at::Tensor& len, const at::Tensor& seg, const at::Tensor& seg_c0,
                      const at::Tensor& seg_nc) {
  ChunkTable ct;
  ct.nchunks = (int32_t)begin.numel();
  ct.nseg = (int32_t)seg_c0.numel();
  ct.begin = vec_ptr<int64_t>(fn, "chunk begin", begin, like, ct.nchunks);
  ct.len = vec_ptr<int32_t>(fn, "chunk len", len, like, ct.nchunks);
  ct.seg = vec_ptr<int32_t>(fn, "chunk seg", seg, like, ct.nchunks);
  ct.seg_c0 = vec_ptr<int32_t>(fn, "seg_c0", seg_c0, like, ct.nseg);
  ct.seg_nc = vec_ptr<int32_t>(fn, "seg_nc", seg_nc, like, ct.nseg);
  return ct;
}

void lars_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& mom,
               const OptTensor& model, const at::Tensor& cbeg, const at::Tensor& clen,
               const at::Tensor& cseg, const at::Tensor& seg_c0, const at::Tensor& seg_nc,
               const at::Tensor& sflag, const at::Tensor& partial, const at::Tensor& norms,
               double lr, double momentum, double wd, double eta, double gscale, double eps,
               bool first, const OptTensor& dyn, const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("lars_step", g, w, model, dyn, skip, gclip, false);
  float* mp = vec_ptr("lars_step", "momentum", mom, g, g.numel());
  ChunkTable ct = make_table("lars_step", g, cbeg, clen, cseg, seg_c0, seg_nc);
  int32_t* fp = vec_ptr<int32_t>("lars_step", "sflag", sflag, g, ct.nseg, true);
  float* pp = vec_ptr("lars_step", "partial", partial, g, 2 * (int64_t)ct.nchunks, true);
  float* np = vec_ptr("lars_step", "norms", norms, g, 2 * (int64_t)ct.nseg, true);
  c10::DeviceGuard guard(g.device());
  mv_launch_lars(g.data_ptr(), dtype_code(g), s.w, mp, s.model, s.model_dt, ct, fp, pp, np,
                 (float)lr, (float)momentum, (float)wd, (float)eta, (float)gscale, (float)eps, first,
                 s.dyn, s.skip, s.gclip, cur_stream());
}

void lars_step(at::Tensor g, at::Tensor w, at::Tensor mom, c10::optional<at::Tensor> model,
               at::Tensor cbeg, at::Tensor clen, at::Tensor cseg, at::Tensor seg_c0,
               at::Tensor seg_nc, at::Tensor sflag, at::Tensor partial, at::Tensor norms, double lr,
               double momentum, double wd, double eta, double gscale, double eps, bool first,
               c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip) {
  lars_impl(g, w, mom, model, cbeg, clen, cseg, seg_c0, seg_nc, sflag, partial, norms, lr,
            momentum, wd, eta, gscale, eps, first, dyn, skip, kNoClip);
}

void lars_step_clip(at::Tensor g, at::Tensor w, at::Tensor mom, c10::optional<at::Tensor> model,
                    at::Tensor cbeg, at::Tensor clen, at::Tensor cseg, at::Tensor seg_c0,
                    at::Tensor seg_nc, at::Tensor sflag, at::Tensor partial, at::Tensor norms,
                    double lr, double momentum, double wd, double eta, double gscale, double eps,
                    bool first, c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                    at::Tensor gclip) {
  lars_impl(g, w, mom, model, cbeg, clen, cseg, seg_c0, seg_nc, sflag, partial, norms, lr,
            momentum, wd, eta, gscale, eps, first, dyn, skip, gclip);
}

void lamb_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& m, const at::Tensor& v,
               const OptTensor& model, const at::Tensor& cbeg, const at::Tensor& clen,
               const at::Tensor& cseg, const at::Tensor& seg_c0, const at::Tensor& seg_nc,
               const at::Tensor& sflag, const at::Tensor& partial, const at::Tensor& norms,
               double lr, double b1, double b2, double eps, double wd, double gscale, int64_t step,
               const OptTensor& dyn, const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("lamb_step", g, w, model, dyn, skip, gclip, false);
  float* mp = vec_ptr("lamb_step", "exp_avg", m, g, g.numel());
  float* vp = vec_ptr("lamb_step", "exp_avg_sq", v, g, g.numel());
  ChunkTable ct = make_table("lamb_step", g, cbeg, clen, cseg, seg_c0, seg_nc);
  int32_t* fp = vec_ptr<int32_t>("lamb_step", "sflag", sflag, g, ct.nseg, true);
  float* pp = vec_ptr("lamb_step", "partial", partial, g, 2 * (int64_t)ct.nchunks, true);
  float* np = vec_ptr("lamb_step", "norms", norms, g, 2 * (int64_t)ct.nseg, true);
  TORCH_CHECK(step >= 1, "lamb_step: step must be >= 1");
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  c10::DeviceGuard guard(g.device());
  mv_launch_lamb(g.data_ptr(), dtype_code(g), s.w, mp, vp, s.model, s.model_dt, ct, fp, pp, np,
                 (float)lr, b1, b2, (float)eps, (float)wd, (float)gscale, (float)bc1, (float)bc2,
                 s.dyn, s.skip, s.gclip, cur_stream());
}

void lamb_step(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v,
               c10::optional<at::Tensor> model, at::Tensor cbeg, at::Tensor clen, at::Tensor cseg,
               at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor sflag, at::Tensor partial,
               at::Tensor norms, double lr, double b1, double b2, double eps, double wd,
               double gscale, int64_t step, c10::optional<at::Tensor> dyn,
               c10::optional<at::Tensor> skip) {
  lamb_impl(g, w, m, v, model, cbeg, clen, cseg, seg_c0, seg_nc, sflag, partial, norms, lr, b1, b2,
            eps, wd, gscale, step, dyn, skip, kNoClip);
}

void lamb_step_clip(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v,
                    c10::optional<at::Tensor> model, at::Tensor cbeg, at::Tensor clen,
                    at::Tensor cseg, at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor sflag,
                    at::Tensor partial, at::Tensor norms, double lr, double b1, double b2,
                    double eps, double wd, double gscale, int64_t step,
                    c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                    at::Tensor gclip) {
  lamb_impl(g, w, m, v, model, cbeg, clen, cseg, seg_c0, seg_nc, sflag, partial, norms, lr, b1, b2,
            eps, wd, gscale, step, dyn, skip, gclip);
}

// RMSprop / Adagrad (mv_adaptive.hip).  grad_avg given: centered; momentum_buffer given: momentum.
void rmsprop_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& sq,
                  const OptTensor& ga, const OptTensor& buf, const OptTensor& model, double lr,
                  double alpha, double eps, double wd, double momentum, double gscale,
                  const OptTensor& dyn, const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("rmsprop_step", g, w, model, dyn, skip, gclip, false);
  float* sp = vec_ptr("rmsprop_step", "square_avg", sq, g, g.numel());
  float* gp = vec_ptr_opt("rmsprop_step", "grad_avg", ga, g, g.numel());
  float* bp = vec_ptr_opt("rmsprop_step", "momentum_buffer", buf, g, g.numel());
  TORCH_CHECK(bp != nullptr || momentum == 0.0,
              "rmsprop_step: momentum_buffer must be given when momentum != 0");
  c10::DeviceGuard guard(g.device());
  mv_launch_rmsprop(g.data_ptr(), dtype_code(g), s.w, sp, gp, bp, s.model, s.model_dt, g.numel(),
                    (float)lr, alpha, (float)eps, (float)wd, (float)momentum, (float)gscale, s.dyn,
                    s.skip, s.gclip, cur_stream());
}

void rmsprop_step(at::Tensor g, at::Tensor w, at::Tensor sq, c10::optional<at::Tensor> ga,
                  c10::optional<at::Tensor> buf, c10::optional<at::Tensor> model, double lr,
                  double alpha, double eps, double wd, double momentum, double gscale,
                  c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip) {
  rmsprop_impl(g, w, sq, ga, buf, model, lr, alpha, eps, wd, momentum, gscale, dyn, skip, kNoClip);
}

void rmsprop_step_clip(at::Tensor g, at::Tensor w, at::Tensor sq, c10::optional<at::Tensor> ga,
                       c10::optional<at::Tensor> buf, c10::optional<at::Tensor> model, double lr,
                       double alpha, double eps, double wd, double momentum, double gscale,
                       c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                       at::Tensor gclip) {
  rmsprop_impl(g, w, sq, ga, buf, model, lr, alpha, eps, wd, momentum, gscale, dyn, skip, gclip);
}

void adagrad_impl(const at::Tensor& g, const at::Tensor& w, const at::Tensor& sum,
                  const OptTensor& model, double lr, double eps, double wd, double gscale,
                  const OptTensor& dyn, const OptTensor& skip, const OptTensor& gclip) {
  const StepArgs s = step_args("adagrad_step", g, w, model, dyn, skip, gclip, false);
  float* sp = vec_ptr("adagrad_step", "sum", sum, g, g.numel());
  c10::DeviceGuard guard(g.device());
  mv_launch_adagrad(g.data_ptr(), dtype_code(g), s.w, sp, s.model, s.model_dt, g.numel(),
                    (float)lr, (float)eps, (float)wd, (float)gscale, s.dyn, s.skip, s.gclip,
                    cur_stream());
}

void adagrad_step(at::Tensor g, at::Tensor w, at::Tensor sum, c10::optional<at::Tensor> model,
                  double lr, double eps, double wd, double gscale, c10::optional<at::Tensor> dyn,
                  c10::optional<at::Tensor> skip) {
  adagrad_impl(g, w, sum, model, lr, eps, wd, gscale, dyn, skip, kNoClip);
}

void adagrad_step_clip(at::Tensor g, at::Tensor w, at::Tensor sum, c10::optional<at::Tensor> model,
                       double lr, double eps, double wd, double gscale,
                       c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                       at::Tensor gclip) {
  adagrad_impl(g, w, sum, model, lr, eps, wd, gscale, dyn, skip, gclip);
}

// Adam with amsgrad, Adamax and NAdam (mv_adamfam.hip).  One entry point each: dyn, skip and
// gclip are trailing optional operands.
void adam_amsgrad_step(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v, at::Tensor vmax,
                       c10::optional<at::Tensor> model, double lr, double b1, double b2, double eps,
                       double wd, double gscale, int64_t step, bool adamw, bool keras_eps,
                       c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                       c10::optional<at::Tensor> gclip) {
  const char* fn = "adam_amsgrad_step";
  const StepArgs s = step_args(fn, g, w, model, dyn, skip, gclip, false);
  float* mp = vec_ptr(fn, "exp_avg", m, g, g.numel());
  float* vp = vec_ptr(fn, "exp_avg_sq", v, g, g.numel());
  float* xp = vec_ptr(fn, "max_exp_avg_sq", vmax, g, g.numel());
  TORCH_CHECK(step >= 1, fn, ": step must be >= 1");
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  c10::DeviceGuard guard(g.device());
  mv_launch_adam_amsgrad(g.data_ptr(), dtype_code(g), s.w, mp, vp, xp, s.model, s.model_dt,
                         g.numel(), (float)lr, b1, b2, (float)eps, (float)wd, (float)gscale,
                         (float)bc1, (float)bc2, adamw, keras_eps, s.dyn, s.skip, s.gclip,
                         cur_stream());
}

void adamax_step(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor u,
                 c10::optional<at::Tensor> model, double lr, double b1, double b2, double eps,
                 double wd, double gscale, int64_t step, bool keras_eps,
                 c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                 c10::optional<at::Tensor> gclip) {
  const char* fn = "adamax_step";
  const StepArgs s = step_args(fn, g, w, model, dyn, skip, gclip, false);
  float* mp = vec_ptr(fn, "exp_avg", m, g, g.numel());
  float* up = vec_ptr(fn, "exp_inf", u, g, g.numel());
  TORCH_CHECK(step >= 1, fn, ": step must be >= 1");
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  c10::DeviceGuard guard(g.device());
  mv_launch_adamax(g.data_ptr(), dtype_code(g), s.w, mp, up, s.model, s.model_dt, g.numel(),
                   (float)lr, b1, b2, (float)eps, (float)wd, (float)gscale, (float)bc1, keras_eps,
                   s.dyn, s.skip, s.gclip, cur_stream());
}

// cg = (1 - mu_t) / (1 - P_t), cm = mu_{t+1} / (1 - P_t mu_{t+1}) and bc2 = 1 - b2^t come from
// the caller, which owns the momentum schedule; each is rounded to fp32 once here.
void nadam_step(at::Tensor g, at::Tensor w, at::Tensor m, at::Tensor v,
                c10::optional<at::Tensor> model, double lr, double b1, double b2, double eps,
                double wd, double gscale, double cg, double cm, double bc2, bool adamw,
                c10::optional<at::Tensor> dyn, c10::optional<at::Tensor> skip,
                c10::optional<at::Tensor> gclip) {
  const char* fn = "nadam_step";
  const StepArgs s = step_args(fn, g, w, model, dyn, skip, gclip, false);
  float* mp = vec_ptr(fn, "exp_avg", m, g, g.numel());
  float* vp = vec_ptr(fn, "exp_avg_sq", v, g, g.numel());
  TORCH_CHECK(bc2 > 0.0, fn, ": bc2 must be > 0");
  c10::DeviceGuard guard(g.device());
  mv_launch_nadam(g.data_ptr(), dtype_code(g), s.w, mp, vp, s.model, s.model_dt, g.numel(),
                  (float)lr, b1, b2, (float)eps, (float)wd, (float)gscale, (float)cg, (float)cm,
                  (float)bc2, adamw, s.dyn, s.skip, s.gclip, cur_stream());
}

// Global gradient-norm clipping (mv_clip.hip).  grad_sumsq writes one fp32 partial per
// 4096-element chunk of x; clip_finalize turns partial[0:total) into clip = [coef, norm].
void grad_sumsq(at::Tensor x, at::Tensor partial, c10::optional<at::Tensor> flag) {
  check_dense("grad_sumsq", "x", x, x);
  const int64_t nchunks = (x.numel() + kChunk - 1) / kChunk;
  float* pp = vec_ptr("grad_sumsq", "partial", partial, x, nchunks, true);
  int* fp = flag_ptr("grad_sumsq", "flag", flag, x);
  c10::DeviceGuard guard(x.device());
  mv_launch_grad_sumsq(x.data_ptr(), dtype_code(x), x.numel(), pp, fp, cur_stream());
}

void clip_finalize(at::Tensor partial, int64_t total, double gscale, double max_norm,
                   at::Tensor clip) {
  TORCH_CHECK(total >= 0, "clip_finalize: total must be >= 0");
  const float* pp = vec_ptr("clip_finalize", "partial", partial, partial, total, true);
  float* cp = vec_ptr("clip_finalize", "clip", clip, partial, 2, true);
  c10::DeviceGuard guard(partial.device());
  mv_launch_clip_finalize(pp, total, gscale, max_norm, cp, cur_stream());
}

// Weight averaging (mv_ema.hip) over the flat fp32 ranges w (master) and e (average) of equal
// length, at any offset; model is the optional low-precision copy of w.
struct EmaArgs {
  float* w;
  float* e;
  void* model = nullptr;
  int model_dt = 0;
  const int* skip;
};

EmaArgs ema_args(const char* fn, const at::Tensor& w, const at::Tensor& e, const OptTensor& model,
                 const OptTensor& skip) {
  EmaArgs s;
  s.w = vec_ptr(fn, "master", w, w, w.numel());
  s.e = vec_ptr(fn, "ema", e, w, w.numel());
  if (given(model)) {
    check_dense(fn, "model", *model, w);
    TORCH_CHECK(model->numel() == w.numel(), fn, ": model must hold exactly ", w.numel(),
                " elements, not ", model->numel());
    s.model = model->data_ptr();
    s.model_dt = dtype_code(*model);
  }
  s.skip = flag_ptr(fn, "skip", skip, w);
  return s;
}

void ema_update(at::Tensor w, at::Tensor e, double decay, c10::optional<at::Tensor> skip) {
  const EmaArgs s = ema_args("ema_update", w, e, c10::nullopt, skip);
  TORCH_CHECK(decay >= 0.0 && decay < 1.0, "ema_update: decay must be in [0, 1), not ", decay);
  c10::DeviceGuard guard(w.device());
  // 1 - decay in double, rounded to fp32 once
  mv_launch_ema_update(s.w, s.e, w.numel(), (float)(1.0 - decay), s.skip, cur_stream());
}

void ema_swap(at::Tensor w, at::Tensor e, c10::optional<at::Tensor> model,
              c10::optional<at::Tensor> skip) {
  const EmaArgs s = ema_args("ema_swap", w, e, model, skip);
  c10::DeviceGuard guard(w.device());
  mv_launch_ema_swap(s.w, s.e, s.model, s.model_dt, w.numel(), s.skip, cur_stream());
}

void ema_overwrite(at::Tensor w, at::Tensor e, c10::optional<at::Tensor> model,
                   c10::optional<at::Tensor> skip) {
  const EmaArgs s = ema_args("ema_overwrite", w, e, model, skip);
  c10::DeviceGuard guard(w.device());
  mv_launch_ema_overwrite(s.w, s.e, s.model, s.model_dt, w.numel(), s.skip, cur_stream());
}

void seg_dot3(at::Tensor a, at::Tensor b, at::Tensor cbeg, at::Tensor clen, at::Tensor cseg,
              at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor partial, at::Tensor out,
              bool swap) {
  check_dense("seg_dot3", "a", a, a);
  check_dense("seg_dot3", "b", b, a);
  TORCH_CHECK(a.numel() == b.numel(), "seg_dot3: a/b numel mismatch");
  TORCH_CHECK(a.scalar_type() == b.scalar_type() || a.scalar_type() == at::kFloat,
              "seg_dot3: a must match b or be fp32");
  ChunkTable ct = make_table("seg_dot3", a, cbeg, clen, cseg, seg_c0, seg_nc);
  float* pp = vec_ptr("seg_dot3", "partial", partial, a, 3 * (int64_t)ct.nchunks, true);
  float* op = vec_ptr("seg_dot3", "out", out, a, 3 * (int64_t)ct.nseg, true);
  c10::DeviceGuard guard(a.device());
  if (a.scalar_type() == b.scalar_type())
    mv_launch_seg_dot3(a.data_ptr(), b.data_ptr(), dtype_code(a), ct, pp, op, swap ? 1 : 0,
                       cur_stream());
  else
    mv_launch_seg_dot3_f(a.data_ptr<float>(), b.data_ptr(), dtype_code(b), ct, pp, op,
                         swap ? 1 : 0, cur_stream());
}

void adasum_merge(at::Tensor fin, at::Tensor f, at::Tensor r, at::Tensor cbeg, at::Tensor clen,
                  at::Tensor cseg, at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor rows,
                  int64_t nrows, bool swap, c10::optional<at::Tensor> emit, int64_t elo,
                  int64_t ehi) {
  check_dense("adasum_merge", "fin", fin, fin);
  float* fp = vec_ptr("adasum_merge", "f", f, fin, fin.numel());
  check_dense("adasum_merge", "r", r, fin);
  TORCH_CHECK(r.numel() == f.numel(), "adasum_merge: size mismatch");
  TORCH_CHECK(fin.scalar_type() == at::kFloat || fin.scalar_type() == r.scalar_type(),
              "adasum_merge: fin must be fp32 or the wire dtype");
  ChunkTable ct = make_table("adasum_merge", fin, cbeg, clen, cseg, seg_c0, seg_nc);
  TORCH_CHECK(nrows >= 1, "adasum_merge: nrows must be >= 1");
  float* rp = vec_ptr("adasum_merge", "rows", rows, fin, nrows * 3 * (int64_t)ct.nseg, true);
  void* ep = nullptr;
  if (given(emit)) {
    check_dense("adasum_merge", "emit", *emit, fin);
    TORCH_CHECK(emit->scalar_type() == r.scalar_type() && emit->numel() == f.numel(),
                "adasum_merge: emit must be a full-length wire-dtype buffer");
    TORCH_CHECK(0 <= elo && elo <= ehi && ehi <= f.numel(), "adasum_merge: emit range");
    ep = emit->data_ptr();
  }
  c10::DeviceGuard guard(f.device());
  mv_launch_adasum_merge(fin.data_ptr(), dtype_code(fin), fp, r.data_ptr(), dtype_code(r), ct, rp,
                         (int)nrows, (int)(rows.numel() / nrows), swap ? 1 : 0, ep, elo, ehi,
                         cur_stream());
}

void adasum_combine(at::Tensor a, at::Tensor b, at::Tensor cbeg, at::Tensor clen, at::Tensor cseg,
                    at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor dots) {
  check_dense("adasum_combine", "a", a, a);
  check_dense("adasum_combine", "b", b, a);
  TORCH_CHECK(a.numel() == b.numel() && a.scalar_type() == b.scalar_type(),
              "adasum_combine: a/b mismatch");
  ChunkTable ct = make_table("adasum_combine", a, cbeg, clen, cseg, seg_c0, seg_nc);
  float* dp = vec_ptr("adasum_combine", "dots", dots, a, 3 * (int64_t)ct.nseg, true);
  c10::DeviceGuard guard(a.device());
  mv_launch_adasum_combine(a.data_ptr(), b.data_ptr(), dtype_code(a), ct, dp, cur_stream());
}

void adasum_fcombine(at::Tensor f, at::Tensor r, at::Tensor cbeg, at::Tensor clen, at::Tensor cseg,
                     at::Tensor seg_c0, at::Tensor seg_nc, at::Tensor dots, bool swap) {
  float* fp = vec_ptr("adasum_fcombine", "f", f, f, f.numel());
  check_dense("adasum_fcombine", "r", r, f);
  TORCH_CHECK(f.numel() == r.numel(), "adasum_fcombine: f/r numel mismatch");
  ChunkTable ct = make_table("adasum_fcombine", f, cbeg, clen, cseg, seg_c0, seg_nc);
  float* dp = vec_ptr("adasum_fcombine", "dots", dots, f, 3 * (int64_t)ct.nseg, true);
  c10::DeviceGuard guard(f.device());
  mv_launch_adasum_fcombine(fp, r.data_ptr(), dtype_code(r), ct, dp, swap ? 1 : 0, cur_stream());
}

}  // namespace

void bind_optim(pybind11::module_& m) {
  m.attr("CHUNK") = kChunk;
  m.attr("MAX_TENSORS_PER_LAUNCH") = kMvMaxTensors;
  m.def("mt_copy", &mt_copy, "multi-tensor pack/unpack with fused cast+scale");
  m.def("flat_cast", &flat_cast, "flat cast + scale (compress/decompress)");
  m.def("nonfinite_scan", &nonfinite_scan, "flag |= any non-finite element (read-only)");
  m.def("sgd_step", &sgd_step, "fused flat SGD(+momentum, nesterov) step");
  m.def("adam_step", &adam_step, "fused flat Adam/AdamW step");
  m.def("adadelta_step", &adadelta_step, "fused flat Adadelta step");
  m.def("lars_step", &lars_step, "fused segmented LARS step");
  // LAMB has a namespace of its own: mivod._mvk._lamb
  pybind11::module_ lb = m.def_submodule(
      "_lamb", "LAMB: Adam moments with a per-segment trust ratio on the flat-arena path");
  lb.def("lamb_step", &lamb_step, "fused segmented LAMB step");
  // so have RMSprop and Adagrad: mivod._mvk._adaptive
  pybind11::module_ ad = m.def_submodule(
      "_adaptive", "RMSprop and Adagrad steps on the flat-arena path");
  ad.def("rmsprop_step", &rmsprop_step, "fused flat RMSprop step (centered / momentum optional)");
  ad.def("adagrad_step", &adagrad_step, "fused flat Adagrad step");
  // and the rest of the Adam family: mivod._mvk._adamfam (dyn, skip and gclip all optional)
  pybind11::module_ af = m.def_submodule(
      "_adamfam", "Adam with amsgrad, Adamax and NAdam steps on the flat-arena path");
  af.def("adam_amsgrad_step", &adam_amsgrad_step,
         "fused flat Adam/AdamW step with amsgrad (max_exp_avg_sq in the denominator)");
  af.def("adamax_step", &adamax_step, "fused flat Adamax step");
  af.def("nadam_step", &nadam_step, "fused flat NAdam step");
  // and global gradient-norm clipping: mivod._mvk._clip, the norm kernels and every step with
  // the device clip coefficient as one more trailing operand
  pybind11::module_ cl = m.def_submodule(
      "_clip", "global gradient-norm clipping (max_grad_norm) on the flat-arena path");
  cl.def("grad_sumsq", &grad_sumsq,
         "partial[b] = fp32 sum of squares of chunk b (deterministic); flag |= any non-finite");
  cl.def("clip_finalize", &clip_finalize,
         "clip = [min(1, max_norm / (norm + 1e-6)), norm], norm = gscale * sqrt(sum partial)");
  cl.def("sgd_step", &sgd_step_clip, "sgd_step with gscale *= gclip[0] on the device");
  cl.def("adam_step", &adam_step_clip, "adam_step with gscale *= gclip[0] on the device");
  cl.def("adadelta_step", &adadelta_step_clip,
         "adadelta_step with gscale *= gclip[0] on the device");
  cl.def("lars_step", &lars_step_clip, "lars_step with gscale *= gclip[0] on the device");
  cl.def("lamb_step", &lamb_step_clip, "lamb_step with gscale *= gclip[0] on the device");
  cl.def("rmsprop_step", &rmsprop_step_clip, "rmsprop_step with gscale *= gclip[0] on the device");
  cl.def("adagrad_step", &adagrad_step_clip, "adagrad_step with gscale *= gclip[0] on the device");
  // and local gradient accumulation in an fp32 arena: mivod._mvk._accum
  pybind11::module_ ac = m.def_submodule(
      "_accum", "fp32 accumulation of backward_passes_per_step micro-batch gradients");
  ac.def("accumulate", &accumulate,
         "acc[off_i : off_i + n_i] = float(t_i) (first) or += float(t_i), one launch");
  ac.def("pack_accumulated", &pack_accumulated,
         "dst[off_i : off_i + n_i] = cast((acc[off_i : off_i + n_i] + float(t_i)) * scale)");
  // and the fp32 moving average of the master weights: mivod._mvk._ema
  pybind11::module_ em = m.def_submodule(
      "_ema", "fp32 exponential moving average of the master weights (ema_decay)");
  em.def("ema_update", &ema_update,
         "e = e + fp32(1 - decay) * (w - e); e = w where fp32(1 - decay) == 1");
  em.def("ema_swap", &ema_swap, "(w, e) = (e, w); model = cast(new w)");
  em.def("ema_overwrite", &ema_overwrite, "w = e; model = cast(e)");
  m.def("seg_dot3", &seg_dot3, "per-segment (a.b, |a|^2, |b|^2) (swap: (a.b, |b|^2, |a|^2))");
  m.def("adasum_merge", &adasum_merge,
        "one vector-halving Adasum level: merge with fixed-order group Gram sums + fused wire cast");
  m.def("adasum_combine", &adasum_combine, "per-segment Adasum merge a <- ca*a + cb*b");
  m.def("adasum_fcombine", &adasum_fcombine,
        "vector-halving Adasum merge on the fp32 running sum f <- cf*f + cr*r");
}
