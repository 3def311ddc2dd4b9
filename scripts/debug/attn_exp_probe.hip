// Diagnostic: the short attention forward (mv_attn.hip fwd_short_kernel) on pseudo-random
// bf16 q/k/v (b 2 x s 128 x h 4 and b 64 x s 128 x h 16), counting NaN outputs, and for the
// first NaN row printing its softmax state (MV_ATTN_PROBE).  Build both exp forms:
//   for e in 0 1; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -DMV_ATTN_RAW_EXP=$e \
//     -DMV_ATTN_PROBE -I csrc/kernels scripts/debug/attn_exp_probe.hip -o /tmp/attn_probe_$e; done
#include "../../csrc/kernels/mv_attn.hip"
#include "../../csrc/kernels/mv_attn_seg.hip"      // mv_attn_fwd links against the segmented launchers

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

static float gauss(uint32_t i, uint32_t seed) {
  auto h = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; };
  const float u1 = ((h(i * 2 + seed) >> 8) + 1) / 16777217.f, u2 = (h(i * 2 + 1 + seed) >> 8) / 16777216.f;
  return std::sqrt(-2.f * std::log(u1)) * std::cos(6.2831853f * u2);
}

int main() {
  const int cfg[2][3] = {{2, 128, 4}, {64, 128, 16}};
  for (int ci = 0; ci < 2; ++ci) {
    const int b = cfg[ci][0], s = cfg[ci][1], h = cfg[ci][2];
    const size_t nq = (size_t)b * s * 3 * h * 64, no = (size_t)b * s * h * 64;
    std::vector<__bf16> hq(nq);
    for (size_t i = 0; i < nq; ++i) hq[i] = (__bf16)(1.5f * gauss((uint32_t)i, 12345u + ci));
    __bf16 *dq, *dout;
    float* dlse;
    CK(hipMalloc(&dq, nq * 2));
    CK(hipMalloc(&dout, no * 2));
    CK(hipMalloc(&dlse, (size_t)b * h * s * 4));
    CK(hipMemcpy(dq, hq.data(), nq * 2, hipMemcpyHostToDevice));
    AttnParams p{};
    p.qkv = dq; p.out = dout; p.lse = dlse; p.mask = nullptr;
    p.b = b; p.s = s; p.h = h; p.scale_log2 = 1.4426950408889634f / 8.f;
    p.p_drop = 0.f; p.seed = 7; p.thresh = 0;
    for (int pass = 0; pass < 2; ++pass) {
      mv_attn_fwd(p, 0);
      CK(hipDeviceSynchronize());
      std::vector<__bf16> ho(no);
      CK(hipMemcpy(ho.data(), dout, no * 2, hipMemcpyDeviceToHost));
      size_t nan = 0;
      int fb = -1, fq = -1;
      for (size_t i = 0; i < no; ++i) {
        const float v = (float)ho[i];
        if (v != v) {
          if (!nan) {
            const size_t row = i / (h * 64);
            fb = (int)((row / s) * h + (i / 64) % h);
            fq = (int)(row % s);
          }
          ++nan;
        }
      }
      std::printf("RAW_EXP %d b %d s %d h %d pass %d: %zu NaN of %zu (first bh %d q %d)\n",
                  MV_ATTN_RAW_EXP, b, s, h, pass, nan, no, fb, fq);
      if (!nan || pass) break;
      CK(hipMemcpyToSymbol(HIP_SYMBOL(mv::attn::g_probe_bh), &fb, sizeof(int)));
      CK(hipMemcpyToSymbol(HIP_SYMBOL(mv::attn::g_probe_q), &fq, sizeof(int)));
    }
    CK(hipFree(dq)); CK(hipFree(dout)); CK(hipFree(dlse));
  }
  return 0;
}
