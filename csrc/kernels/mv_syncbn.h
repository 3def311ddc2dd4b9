// Host launchers for SyncBatchNorm's cross-rank middle (mv_syncbn.hip): the kernels that
// sit between mv_bn.h's streaming passes and the two collectives of a synchronized BN.
//
//   forward   mv_bn_stats_pass -> mv_syncbn_record -> [allgather] -> mv_syncbn_merge
//             -> mv_bn_apply
//   backward  mv_bn_bwd_reduce_pass -> mv_syncbn_bwd_local -> [allreduce sum]
//             -> mv_syncbn_bwd_coeffs -> mv_bn_bwd_dx_pass
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One rank's statistics record, in 32-bit words (a fixed size for a given C, so ranks with
// different batch sizes meet in one equal-size allgather):
//   [0, C)    fp32  s1 = sum (x - shift)
//   [C, 2C)   fp32  s2 = sum (x - shift)^2
//   [2C, 3C)  fp32  shift (this rank's running mean, or 0)
//   3C, 3C+1  int64 rows summed (an fp32 count is inexact from 2^24 rows)
//   3C+2, +3  0     (keeps records 16-byte aligned)
inline int64_t mv_syncbn_record_words(int C) { return 3 * (int64_t)C + 4; }

// [P][2][C] statistics partials of M rows around shift (null: 0) -> rec
void mv_syncbn_record(const float* partial, int P, int64_t M, int C, const float* shift,
                      int32_t* rec, hipStream_t st);

// N gathered records -> vec [4][C] {mean, invstd, scale, bias} as finalize_fwd_kernel writes
// it, the running statistics updated with the global count (both null: not tracked), and
// that count in *count for the backward
void mv_syncbn_merge(const int32_t* recs, int N, int C, float* rmean, float* rvar,
                     const float* gamma, const float* beta, float momentum, float eps, float* vec,
                     int64_t* count, hipStream_t st);

// [P][2][C] reduce partials -> this rank's dgamma / dbeta (null: not wanted) and
// tot [2][C] = (sum dz, sum dz (x - mean)) over this rank's rows
void mv_syncbn_bwd_local(const float* partial, int P, int C, const float* invstd, float* dgamma,
                         float* dbeta, float* tot, hipStream_t st);

// tot summed over the ranks + the global count -> dx = ca * dz + cb * x + cc
void mv_syncbn_bwd_coeffs(const float* tot, const int64_t* count, int C, const float* mean,
                          const float* invstd, const float* gamma, float* ca, float* cb, float* cc,
                          hipStream_t st);
