// The wave-private-ring GEMM family (gemm_glds_impl.h: mainloop_private, gemm_private_kernel):
// 32 x 48 tiles whose W waves each multiply the whole tile over a K slice of their own, from an
// LDS ring of their own, with no barrier between the first DMA and the last MFMA. Ids
// kGemmPrivate + i (kernels.h) outside the LDS-DMA config table: the family has its own slim
// kernel arguments and refuses what it does not attach. Below it the same rings on 64 x 96 and
// 64 x 80 tiles with the folded-norm finish (gemm_private_wide_kernel), ids kGemmPrivateWide + i.
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

// The 64-row family with the folded-norm finish (gemm_private_wide_kernel): ids kGemmPrivateWide + i,
// tile and W x S from kGemmPrivateWideCfgs (kernels.h).
int gemm_private_wide_waves(int cfg) {
  return cfg >= kGemmPrivateWide && cfg < kGemmPrivateWide + kGemmPrivateWideCount
             ? kGemmPrivateWideCfgs[cfg - kGemmPrivateWide].waves
             : 0;
}

bool gemm_private_wide_takes(const GemmArgs& a, int cfg, int splitk, int ln_mode, bool ranged) {
  return private_wide_takes(gemm_private_wide_waves(cfg), a, splitk, ln_mode, ranged);
}

bool launch_gemm_private_wide(const GemmArgs& a, int cfg, const float* ln_colsum, int ln_mode, float ln_eps,
                              hipStream_t s) {
  // (the same rule as above makes the barrier unmissable: equal K-tile counts, grid == tile count)
  if (!ln_colsum || !gemm_private_wide_takes(a, cfg, 1, ln_mode, false)) return false;
  switch (cfg - kGemmPrivateWide) {
    case 0: launch_private_wide<64, 96, 4, 2>(a, ln_colsum, ln_mode, ln_eps, s); break;
    case 1: launch_private_wide<64, 96, 3, 2>(a, ln_colsum, ln_mode, ln_eps, s); break;
    case 2: launch_private_wide<64, 80, 4, 2>(a, ln_colsum, ln_mode, ln_eps, s); break;
    default: launch_private_wide<64, 80, 3, 2>(a, ln_colsum, ln_mode, ln_eps, s); break;
  }
  return true;
}
