// gemm_quant_host.h: the host-side decisions that the dense quantised GEMMs share (gemm_w8.hip,
// gemm_w8a8.hip, gemm_w4a8.hip): the tile table, split-K limits and workspace, the split a launch
// resolves to, and the config pick. Host code only: each kernel keeps its device code to itself.
#pragma once
#include <cstddef>

namespace quant_host {

// the four tile configs every format instantiates: {128x128, 64x128, 64x64, 32x64}, 2 x 2 waves
constexpr int kNumCfg = 4;
constexpr int kTileM[kNumCfg] = {128, 64, 64, 32};
constexpr int kTileN[kNumCfg] = {128, 128, 64, 64};
constexpr int kMaxSplit = 8;

inline long blocks_for(int M, int N, int c) {
  return (long)((M + kTileM[c] - 1) / kTileM[c]) * ((N + kTileN[c] - 1) / kTileN[c]);
}

// BK: K elements per slice of the format's kernel
inline int max_splitk(int K, int BK) {
  const int kt = (K + BK - 1) / BK;
  return kt < kMaxSplit ? (kt < 1 ? 1 : kt) : kMaxSplit;
}

inline size_t workspace_bytes(int M, int N, int splitk) {
  return splitk > 1 ? (size_t)splitk * M * N * sizeof(float) : 0;
}

// What a launch makes of the requested split: at most one split per slice, no empty split, one
// split without a workspace. kper: K elements per split (a multiple of BK).
struct Split {
  int splitk, kper;
};
inline Split resolve_split(int K, int BK, int want, bool has_workspace) {
  const int kt = (K + BK - 1) / BK;
  int splitk = want < 1 ? 1 : want;
  if (splitk > kt) splitk = kt;
  const int per = (kt + splitk - 1) / splitk;
  splitk = (kt + per - 1) / per;  // no empty split
  if (!has_workspace) splitk = 1;
  return {splitk, (splitk > 1 ? per : kt) * BK};
}

// Fitted to the cold-weight measurements of the GPT-2 and Llama-3-8B layer shapes at M = 512 with
// the W8A16 kernel (benchmarks/bench_gemm_w8.py, profiles/w8/gemm_w8.txt; BK = 64: split_slices 16,
// tail_slices 8); the kernels with 128-element slices keep the rule with the slice counts halved:
//  * 128 x 128 tiles when they alone cover the 256 CUs (gate/up, LM head);
//  * 128 x 128 tiles with a K split when the split grid fills whole rounds of the 512 blocks
//    resident at once (two per CU) and every split keeps >= split_slices slices (Llama's wo and
//    down projections: 128 tiles x 4); a grid that ends in a mostly empty round loses more than
//    the split gains (Llama's QKV: 192 tiles);
//  * otherwise small tiles, several blocks per CU: 64 x 64 when that gives 512 blocks, else
//    32 x 64, K split while the grid is below 512 blocks and >= tail_slices slices per split remain.
inline void pick(int M, int N, int K, int BK, int split_slices, int tail_slices, int* cfg, int* splitk) {
  const int kt = (K + BK - 1) / BK;
  const long b0 = blocks_for(M, N, 0);
  *cfg = 0;
  *splitk = 1;
  if (b0 >= 256) return;
  if (M > 64)
    for (int sk = 2; sk <= kMaxSplit; sk *= 2) {
      if (kt / sk < split_slices) break;
      const long rounds = (b0 * sk + 511) / 512;
      if (b0 * sk >= 512 && b0 * sk * 10 >= rounds * 512 * 9) {
        *splitk = sk;
        return;
      }
    }
  const int c = (M > 32 && blocks_for(M, N, 2) >= 512) ? 2 : 3;
  const long blocks = blocks_for(M, N, c);
  int sk = 1;
  while (sk < kMaxSplit && blocks * sk < 512 && kt / (sk * 2) >= tail_slices) sk *= 2;
  *cfg = c;
  *splitk = sk;
}

}  // namespace quant_host
