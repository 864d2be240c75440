// The wave-private-ring GEMM family (gemm_glds_impl.h: mainloop_private, gemm_private_kernel):
// 32 x 48 tiles whose W waves each multiply the whole tile over a K slice of their own, from an
// LDS ring of their own, with no barrier between the first DMA and the last MFMA. Ids
// kGemmPrivate + i (kernels.h) outside the LDS-DMA config table: the family has its own slim
// kernel arguments and refuses what it does not attach.
#include "gemm_glds_impl.h"

namespace {
constexpr int kWaves[kGemmPrivateCount] = {8, 4, 6, 12};
}

int gemm_private_waves(int cfg) {
  return cfg >= kGemmPrivate && cfg < kGemmPrivate + kGemmPrivateCount ? kWaves[cfg - kGemmPrivate] : 0;
}

bool gemm_private_takes(const GemmArgs& a, int cfg, int splitk, bool folded_norm, bool ranged) {
  return private_takes(gemm_private_waves(cfg), a, splitk, folded_norm, ranged);
}

bool launch_gemm_private(const GemmArgs& a, int cfg, hipStream_t s) {
  // (every wave of a block runs the same K-tile count and the grid is exactly the tile count:
  // what makes the kernel's one barrier unmissable is checked HERE, not assumed)
  if (!gemm_private_takes(a, cfg, 1, false, false)) return false;
  switch (cfg - kGemmPrivate) {
    case 0: launch_private<8, 2>(a, s); break;
    case 1: launch_private<4, 3>(a, s); break;
    case 2: launch_private<6, 2>(a, s); break;
    default: launch_private<12, 1>(a, s); break;
  }
  return true;
}
