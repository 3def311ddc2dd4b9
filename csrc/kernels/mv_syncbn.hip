// SyncBatchNorm's cross-rank middle for the fused NHWC BatchNorm of mv_bn.hip.
//
// A synchronized BN normalizes with the statistics of every rank's rows.  The streaming
// passes over the activation are mv_bn.hip's (statistics, apply, backward reduce, dx);
// what differs is the finalize between them, which here is split around a collective:
//
//   record      this rank's [P][2][C] partials -> one fixed-size record (sums, the shift
//               they were taken around, the exact row count)
//   merge       the N gathered records -> global mean / invstd / scale / bias, the running
//               statistics and the global count; Chan's pairwise update in rank order, so
//               every rank computes the same bits from the same gathered bytes
//   bwd_local   the backward reduce's partials -> local dgamma / dbeta (the optimizer's
//               allreduce averages those) and the [2][C] totals that are summed over ranks
//   bwd_coeffs  the summed totals and the global count -> the dx pass's coefficients
//
// All four are latency-bound (C <= 2048 channels, N = world size): no host round trip,
// the count stays on the device, one launch each.
#include "mv_common.h"
#include "mv_bn_fin.h"
#include "mv_syncbn.h"

namespace mv {
namespace syncbn {

using bn::kFinCh;

constexpr int kChBlock = kWave;   // merge / coeffs: one channel per lane, one wave per workgroup

__global__ __launch_bounds__(kBlock) void record_kernel(const float* __restrict__ partial, int P,
                                                         int64_t M, int C,
                                                         const float* __restrict__ shift,
                                                         int32_t* __restrict__ rec) {
  const int ch = blockIdx.x * kFinCh + threadIdx.x % kFinCh;
  float s1 = 0.f, s2 = 0.f;
  bn::fin_reduce(partial, P, C, ch, &s1, &s2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t* cnt = reinterpret_cast<int64_t*>(rec + 3 * (int64_t)C);
    cnt[0] = M;
    cnt[1] = 0;
  }
  if (threadIdx.x / kFinCh != 0 || ch >= C) return;
  float* f = reinterpret_cast<float*>(rec);
  f[ch] = s1;
  f[C + ch] = s2;
  f[2 * C + ch] = shift ? shift[ch] : 0.f;
}

__global__ __launch_bounds__(kChBlock) void merge_kernel(
    const int32_t* __restrict__ recs, int N, int C, float* __restrict__ rmean,
    float* __restrict__ rvar, const float* __restrict__ gamma, const float* __restrict__ beta,
    float momentum, float eps, float* __restrict__ vec, int64_t* __restrict__ count) {
  const int ch = blockIdx.x * kChBlock + threadIdx.x;
  const int64_t words = 3 * (int64_t)C + 4;
  int64_t n = 0;
  float mean = 0.f, m2 = 0.f;
  if (ch < C) {
    for (int r = 0; r < N; ++r) {
      const int32_t* q = recs + r * words;
      const int64_t nr = *reinterpret_cast<const int64_t*>(q + 3 * (int64_t)C);
      if (nr <= 0) continue;          // an empty rank: nothing to add, nothing to divide
      const float* f = reinterpret_cast<const float*>(q);
      const float s1 = f[ch], s2 = f[C + ch], sh = f[2 * C + ch];
      const float fr = (float)nr;
      const float ms = s1 / fr;
      const float mr = sh + ms;
      const float m2r = fmaxf(__builtin_fmaf(-s1, ms, s2), 0.f);
      if (n == 0) {
        n = nr;
        mean = mr;
        m2 = m2r;
        continue;
      }
      // Chan et al.: (n, mean, M2) + (nr, mr, m2r)
      const float fa = (float)n;
      n += nr;
      const float w = fr / (float)n;
      const float d = mr - mean;
      mean += d * w;
      m2 += m2r + d * d * (fa * w);
    }
  }
  if (ch >= C) return;
  if (ch == 0) *count = n;   // every channel walks the same counts
  const float var = n > 0 ? m2 / (float)n : 0.f;
  const float invstd = 1.f / sqrtf(var + eps);
  vec[ch] = mean;
  vec[C + ch] = invstd;
  if (rmean && n > 0) {
    const float unb = n > 1 ? var * (float)n / (float)(n - 1) : var;
    rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * mean;
    rvar[ch] = (1.f - momentum) * rvar[ch] + momentum * unb;
  }
  const float sc = (gamma ? gamma[ch] : 1.f) * invstd;
  vec[2 * C + ch] = sc;
  vec[3 * C + ch] = (beta ? beta[ch] : 0.f) - mean * sc;
}

__global__ __launch_bounds__(kBlock) void bwd_local_kernel(const float* __restrict__ partial, int P,
                                                            int C, const float* __restrict__ invstd,
                                                            float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta,
                                                            float* __restrict__ tot) {
  const int ch = blockIdx.x * kFinCh + threadIdx.x % kFinCh;
  float sdz = 0.f, sdzx = 0.f;
  bn::fin_reduce(partial, P, C, ch, &sdz, &sdzx);
  if (threadIdx.x / kFinCh != 0 || ch >= C) return;
  if (dgamma) dgamma[ch] = sdzx * invstd[ch];
  if (dbeta) dbeta[ch] = sdz;
  tot[ch] = sdz;
  tot[C + ch] = sdzx;
}

// finalize_bwd_kernel's coefficients from global totals and the global count
__global__ __launch_bounds__(kChBlock) void bwd_coeffs_kernel(
    const float* __restrict__ tot, const int64_t* __restrict__ count, int C,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, float* __restrict__ ca, float* __restrict__ cb,
    float* __restrict__ cc) {
  const int ch = blockIdx.x * kChBlock + threadIdx.x;
  if (ch >= C) return;
  const int64_t m = *count;
  const float inv_m = m > 0 ? 1.f / (float)m : 0.f;
  const float sdz = tot[ch], sdzx = tot[C + ch];
  const float is = invstd[ch];
  const float gm = gamma ? gamma[ch] : 1.f;
  const float a = gm * is;
  const float b = -a * is * is * sdzx * inv_m;
  ca[ch] = a;
  cb[ch] = b;
  cc[ch] = -a * sdz * inv_m - b * mean[ch];
}

}  // namespace syncbn
}  // namespace mv

using namespace mv;
using namespace mv::syncbn;

void mv_syncbn_record(const float* partial, int P, int64_t M, int C, const float* shift,
                      int32_t* rec, hipStream_t st) {
  hipLaunchKernelGGL(record_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kBlock), 0, st, partial,
                     P, M, C, shift, rec);
}

void mv_syncbn_merge(const int32_t* recs, int N, int C, float* rmean, float* rvar,
                     const float* gamma, const float* beta, float momentum, float eps, float* vec,
                     int64_t* count, hipStream_t st) {
  hipLaunchKernelGGL(merge_kernel, dim3((C + kChBlock - 1) / kChBlock), dim3(kChBlock), 0, st,
                     recs, N, C, rmean, rvar, gamma, beta, momentum, eps, vec, count);
}

void mv_syncbn_bwd_local(const float* partial, int P, int C, const float* invstd, float* dgamma,
                         float* dbeta, float* tot, hipStream_t st) {
  hipLaunchKernelGGL(bwd_local_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kBlock), 0, st,
                     partial, P, C, invstd, dgamma, dbeta, tot);
}

void mv_syncbn_bwd_coeffs(const float* tot, const int64_t* count, int C, const float* mean,
                          const float* invstd, const float* gamma, float* ca, float* cb, float* cc,
                          hipStream_t st) {
  hipLaunchKernelGGL(bwd_coeffs_kernel, dim3((C + kChBlock - 1) / kChBlock), dim3(kChBlock), 0,
                     st, tot, count, C, mean, invstd, gamma, ca, cb, cc);
}
