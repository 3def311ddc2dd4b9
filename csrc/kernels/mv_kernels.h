// Host-side declarations of the mivod gfx950 kernel launchers (mv_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Multi-tensor table passed by value in the kernel arguments (<= 2 KB).
constexpr int kMvMaxTensors = 64;
struct MtArgs {
  void* ptr[kMvMaxTensors];            // tensor-side pointers
  int64_t numel[kMvMaxTensors];
  int64_t flat_off[kMvMaxTensors];     // element offset in the flat buffer
  int32_t chunk_start[kMvMaxTensors + 1];  // prefix sum of 4096-element chunks
  int32_t ntensors;
};

// Static segment/chunk table of a flat bucket (device pointers).
struct ChunkTable {
  const int64_t* begin;   // [nchunks] element offset of each chunk
  const int32_t* len;     // [nchunks]
  const int32_t* seg;     // [nchunks] owning segment
  const int32_t* seg_c0;  // [nseg] first chunk of segment
  const int32_t* seg_nc;  // [nseg] chunk count of segment
  int32_t nchunks;
  int32_t nseg;
};

void mv_launch_mt_copy(const MtArgs& a, int tensor_dtype, void* flat, int flat_dtype, bool to_flat,
                       float scale, int* found_nonfinite, hipStream_t st);
// flag |= any(!isfinite(x)) (read-only)
void mv_launch_nonfinite_scan(const void* x, int dtype, int64_t n, int* flag, hipStream_t st);
void mv_launch_flat_cast(const void* src, int sd, void* dst, int dd, int64_t n, float scale,
                         int* found_nonfinite, hipStream_t st);
// dampening, b1, b2 and rho arrive as doubles: their complements 1 - x are rounded to fp32 once
void mv_launch_sgd(const void* g, int gd, float* w, float* mom, void* model, int md, int64_t n,
                   float lr, float momentum, double dampening, float wd, float gscale, int nesterov,
                   int first, const float* dyn, const int* skip, const float* gclip,
                   hipStream_t st);
// skip (nullable): device int32; nonzero => the kernel returns without updating
// (fp16-wire overflow guard, identical on every rank after the flag allreduce)
// dyn (nullable): device [lr, first, bc1, bc2] read by the kernel instead of the
// scalar arguments — HIP-graph replayable hyperparameters (mivod/torch/graphs.py)
// gclip (nullable): device fp32 clip coefficient of the step (mv_clip.h); the kernel
// multiplies gscale by gclip[0], one fp32 product, before any element is touched (LARS: in
// both the norm pass and the update, so the trust ratio sees the clipped gradient)
// m, v (Adam) and sq, acc (Adadelta) must not be null: the kernels tell the compiler so
// (__builtin_assume), and a null one is undefined behaviour, not a skipped stream
void mv_launch_adam(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                    int64_t n, float lr, double b1, double b2, float eps, float wd, float gscale,
                    float bc1, float bc2, int adamw, int keras_eps, const float* dyn,
                    const int* skip, const float* gclip, hipStream_t st);
void mv_launch_adadelta(const void* g, int gd, float* w, float* sq, float* acc, void* model, int md,
                        int64_t n, float lr, double rho, float eps, float wd, float gscale,
                        const float* dyn, const int* skip, const float* gclip, hipStream_t st);
void mv_launch_lars(const void* g, int gd, float* w, float* mom, void* model, int md,
                    const ChunkTable& ct, const int32_t* sflag, float* partial, float* norms,
                    float lr, float momentum, float wd, float eta, float gscale, float eps,
                    int first, const float* dyn, const int* skip, const float* gclip,
                    hipStream_t st);
// LAMB: m, v updated and per-chunk (|w|^2, |u|^2) partials, the segment reduce into
// norms[2 * nseg], then w -= lr * trust * u with u recomputed from the stored m, v and w.
// sflag bit0: the segment takes no weight decay and trust 1.  dyn overrides lr, bc1, bc2;
// skip makes both streaming kernels return before they touch w, m, v or the model copy.
void mv_launch_lamb(const void* g, int gd, float* w, float* m, float* v, void* model, int md,
                    const ChunkTable& ct, const int32_t* sflag, float* partial, float* norms,
                    float lr, double b1, double b2, float eps, float wd, float gscale, float bc1,
                    float bc2, const float* dyn, const int* skip, const float* gclip,
                    hipStream_t st);
// swap: store (a.b, |b|^2, |a|^2) (the Adasum level kernels, f holding b)
void mv_launch_seg_dot3(const void* a, const void* b, int dt, const ChunkTable& ct, float* partial,
                        float* out, int swap, hipStream_t st);
void mv_launch_adasum_combine(void* a, const void* b, int dt, const ChunkTable& ct,
                              const float* dots, hipStream_t st);
// Adasum (vector halving): per-segment (a.b, |a|^2, |b|^2) with a fp32 and b any dtype
void mv_launch_seg_dot3_f(const float* a, const void* b, int bdt, const ChunkTable& ct,
                          float* partial, float* out, int swap, hipStream_t st);
// f <- cf*f + cr*r on the fp32 running merge (swap: f holds b instead of a)
void mv_launch_adasum_fcombine(float* f, const void* r, int rdt, const ChunkTable& ct,
                               const float* dots, int swap, hipStream_t st);
// one vector-halving level: f <- cf*fin + cr*r with the Gram terms summed over
// `nrows` rows in fixed order; fin fp32 (== f) or the wire dtype of r; emit
// (nullable, r's dtype) receives cast(f) on [elo, ehi)
void mv_launch_adasum_merge(const void* fin, int fdt, float* f, const void* r, int rdt,
                            const ChunkTable& ct, const float* rows, int nrows, int row_stride,
                            int swap, void* emit, int64_t elo, int64_t ehi, hipStream_t st);
