// W8A16 GEMM on the bf16 MFMA:  C = act(alpha * scale[n] * sum_k A[m][k] * Wq[n][k] + bias[n]) + R
//
//   A  [M][K] bf16 row-major (activations)
//   Wq [N][K] OCP e4m3 bytes (weights, K contiguous), scale [N] fp32 (one per output channel)
//   C, R [M][N] bf16, bias [N] bf16; fp32 accumulation in the MFMA accumulators.
//
// Structure: the register-staged, double-buffered loop of gemm.hip (BK = 64, one barrier per
// K slice) with the weight tile staged as BYTES: a weight row of a slice is 64 B in LDS (half
// the bf16 kernel's), and half the bytes come from HBM. After the LDS read a lane converts its
// 16 e4m3 bytes to bf16 in registers (v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32: every e4m3 value,
// subnormals included, is exactly a bf16 value), so the products are exact and the channel
// scale is applied once, in the epilogue.
//
// K order inside a slice: both MFMA operands may permute k the same way, so lane group
// g = lane >> 4 owns k = 16g .. 16g+15 of the slice — ONE 16-byte LDS read of the weight row
// feeds two MFMA steps (bytes 0..7, then 8..15), and the A operand reads its 16-byte chunks
// 2g and 2g+1 for them.
//
// Operands are swapped (W is the MFMA's A operand): a lane's four accumulator values are four
// CONSECUTIVE output columns of one row, so the epilogue stores 8 bytes per fragment and a
// SwiGLU gate/up pair (weight rows interleaved in blocks of 16) is two fragments of one lane.
//
// LDS swizzles (16-byte chunks): A rows are 128 B, chunk c of row r at c ^ (r & 7) as in
// gemm.hip; W rows are 64 B, chunk c of row r at c ^ ((r >> 2) & 3), which spreads the 16 rows
// of one ds_read_b128 lane group over all 16 chunk slots of 256 B.
//
// Split-K (grid.z): each split writes an fp32 partial slab, a second kernel sums the slabs in
// a fixed order and runs the epilogue — no atomics, bitwise reproducible.
#include "common.h"
#include "gemm_quant_host.h"
#include "gemm_quant_reduce.h"
#include "kernels.h"

namespace {

constexpr int BK = 64;
constexpr int ACH = BK / 8;   // 16-byte chunks per A row of a slice
constexpr int WCH = BK / 16;  // 16-byte chunks per W row of a slice

template <int BM_, int BN_, int WAVES_M, int WAVES_N>
struct W8Cfg {
  static constexpr int BM = BM_, BN = BN_, WM = WAVES_M, WN = WAVES_N;
  static constexpr int T = 64 * WAVES_M * WAVES_N;
  static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  static constexpr int FM = WTM / 16, FN = WTN / 16;
  static constexpr int A_UNITS = BM * ACH, W_UNITS = BN * WCH;
  static constexpr int A_PER = (A_UNITS + T - 1) / T, W_PER = (W_UNITS + T - 1) / T;
  static constexpr int STAGE = A_UNITS + W_UNITS;  // 16-byte units per buffer
  static_assert(FM >= 1 && FN >= 2 && FN % 2 == 0, "wave tile: whole gate/up fragment pairs");
  static_assert(WTN % 32 == 0, "a wave's columns start on a gate/up block pair");
  static_assert(A_UNITS % T == 0 && W_UNITS % T == 0, "whole staging passes");
  static_assert(2 * STAGE * 16 <= 64 * 1024, "static LDS");
};

struct W8Params {
  const bf16* A;
  const uint8_t* W;
  const float* scale;
  bf16* C;
  const bf16* bias;
  const bf16* R;
  float* part;  // split-K: fp32 [splitk][M][N]
  int lda, ldw, ldc, ldr;
  int M, N, K;
  int act;
  float alpha;
  int tiles_m, tiles_n;
  int kper;  // K elements per split (a multiple of BK)
  int pol;   // store8_pol aux bits of the output stores (0, 2 nt, 16 write-through)
};

// the format to gemm_quant_reduce.h
struct W8A16 {
  using Params = W8Params;
  static constexpr bool kRowScale = false, kColScale = true;
};

template <class G>
__global__ __launch_bounds__(G::T) void gemm_w8_kernel(const W8Params p) {
  __shared__ u32x4 smem[2 * G::STAGE];
  constexpr int BM = G::BM, BN = G::BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / G::WN, wn = wave % G::WN;
  const int l16 = lane & 15, g = lane >> 4;
  const int bid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
  const int m0 = (bid % p.tiles_m) * BM, n0 = (bid / p.tiles_m) * BN;  // m fastest: neighbours share W
  const int M = p.M, N = p.N;
  const int kbeg = blockIdx.z * p.kper, kend = min(p.K, kbeg + p.kper);

  f32x4 acc[G::FM][G::FN];
#pragma unroll
  for (int i = 0; i < G::FM; ++i)
#pragma unroll
    for (int j = 0; j < G::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[G::A_PER], rw[G::W_PER];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < G::A_PER; ++i) {
      const int q = tid + i * G::T, row = q / ACH, c = q % ACH;
      const int gm = m0 + row, gk = k0 + c * 8;
      ra[i] = (q < G::A_UNITS && gm < M && gk < kend)
                  ? *reinterpret_cast<const u32x4*>(p.A + (size_t)gm * p.lda + gk)
                  : zero4;
    }
#pragma unroll
    for (int i = 0; i < G::W_PER; ++i) {
      const int q = tid + i * G::T, row = q / WCH, c = q % WCH;
      const int gn = n0 + row, gk = k0 + c * 16;
      rw[i] = (q < G::W_UNITS && gn < N && gk < kend)
                  ? *reinterpret_cast<const u32x4*>(p.W + (size_t)gn * p.ldw + gk)
                  : zero4;
    }
  };
  auto store_tile = [&](int buf) {
    u32x4* s = smem + buf * G::STAGE;
#pragma unroll
    for (int i = 0; i < G::A_PER; ++i) {
      const int q = tid + i * G::T, row = q / ACH, c = q % ACH;
      if (q < G::A_UNITS) s[row * ACH + (c ^ (row & 7))] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < G::W_PER; ++i) {
      const int q = tid + i * G::T, row = q / WCH, c = q % WCH;
      if (q < G::W_UNITS) s[G::A_UNITS + row * WCH + (c ^ ((row >> 2) & 3))] = rw[i];
    }
  };

  const int nk = (kend - kbeg + BK - 1) / BK;  // <= 0: an empty split writes a zero slab
  if (nk > 0) {
    load_tile(kbeg);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kbeg + (kt + 1) * BK);  // in flight under the MFMAs below
    const u32x4* s = smem + cur * G::STAGE;
    u32x4 wraw[G::FN];
#pragma unroll
    for (int j = 0; j < G::FN; ++j) {
      const int row = wn * G::WTN + j * 16 + l16;
      wraw[j] = s[G::A_UNITS + row * WCH + (g ^ ((row >> 2) & 3))];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bf16x8 af[G::FM], wf[G::FN];
#pragma unroll
      for (int i = 0; i < G::FM; ++i) {
        const int row = wm * G::WTM + i * 16 + l16;
        const u32x4 v = s[row * ACH + ((2 * g + h) ^ (row & 7))];
        af[i] = *reinterpret_cast<const bf16x8*>(&v);
      }
#pragma unroll
      for (int j = 0; j < G::FN; ++j) wf[j] = cvt_e4m3x8(wraw[j][2 * h], wraw[j][2 * h + 1]);
#pragma unroll
      for (int i = 0; i < G::FM; ++i)
#pragma unroll
        for (int j = 0; j < G::FN; ++j) acc[i][j] = mfma16x16x32(wf[j], af[i], acc[i][j]);
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // lane: row m0 + wm*WTM + i*16 + l16, columns n0 + wn*WTN + j*16 + 4g .. +3
  if (p.part != nullptr) {
    float* P = p.part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < G::FM; ++i) {
      const int row = m0 + wm * G::WTM + i * 16 + l16;
      if (row >= M) continue;
#pragma unroll
      for (int j = 0; j < G::FN; ++j) {
        const int col = n0 + wn * G::WTN + j * 16 + 4 * g;
        if (N % 4 == 0 && col + 3 < N) {
          *reinterpret_cast<f32x4*>(P + (size_t)row * N + col) = acc[i][j];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < N) P[(size_t)row * N + col + e] = acc[i][j][e];
        }
      }
    }
    return;
  }
  const int ldc = p.ldc, ldr = p.ldr;
  const bf16* __restrict__ R = p.R;
  bf16* __restrict__ C = p.C;
  const bool vec_ok = (ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 7) == 0);
  if (p.act == ACT_SWIGLU) {
    // fragments (2jj, 2jj+1) of a lane: gate and up of the same four output columns
    const int NO = N / 2;
#pragma unroll
    for (int jj = 0; jj < G::FN / 2; ++jj) {
      const int gcol = n0 + wn * G::WTN + jj * 32 + 4 * g;
      const int ocol = (n0 + wn * G::WTN) / 2 + jj * 16 + 4 * g;
      if (ocol >= NO) continue;  // N % 32 == 0: a block pair is inside N or past it as a whole
      float sg[4], su[4], bg[4], bu[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sg[e] = p.alpha * p.scale[gcol + e];
        su[e] = p.alpha * p.scale[gcol + 16 + e];
        bg[e] = p.bias ? bf2f(p.bias[gcol + e]) : 0.f;
        bu[e] = p.bias ? bf2f(p.bias[gcol + 16 + e]) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < G::FM; ++i) {
        const int row = m0 + wm * G::WTM + i * 16 + l16;
        if (row >= M) continue;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = silu(sg[e] * acc[i][2 * jj][e] + bg[e]) * (su[e] * acc[i][2 * jj + 1][e] + bu[e]);
          if (R) v += bf2f(R[(size_t)row * ldr + ocol + e]);
          o[e] = f2bf(v);
        }
        if (vec_ok) {
          store_bf16x4(C, (size_t)row * ldc + ocol, o, p.pol);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) C[(size_t)row * ldc + ocol + e] = o[e];
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < G::FN; ++j) {
    const int col = n0 + wn * G::WTN + j * 16 + 4 * g;
    if (col >= N) continue;
    float sc[4], bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = col + e < N;
      sc[e] = in ? p.alpha * p.scale[col + e] : 0.f;
      bv[e] = (in && p.bias) ? bf2f(p.bias[col + e]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < G::FM; ++i) {
      const int row = m0 + wm * G::WTM + i * 16 + l16;
      if (row >= M) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = apply_act(sc[e] * acc[i][j][e] + bv[e], p.act);
        if (R && col + e < N) v += bf2f(R[(size_t)row * ldr + col + e]);
        o[e] = f2bf(v);
      }
      if (vec_ok && col + 3 < N) {
        store_bf16x4(C, (size_t)row * ldc + col, o, p.pol);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < N) C[(size_t)row * ldc + col + e] = o[e];
      }
    }
  }
}

using W8C0 = W8Cfg<128, 128, 2, 2>;
using W8C1 = W8Cfg<64, 128, 2, 2>;
using W8C2 = W8Cfg<64, 64, 2, 2>;
using W8C3 = W8Cfg<32, 64, 2, 2>;

template <class G>
void launch_cfg(W8Params p, int splitk, hipStream_t s) {
  p.tiles_m = (p.M + G::BM - 1) / G::BM;
  p.tiles_n = (p.N + G::BN - 1) / G::BN;
  hipLaunchKernelGGL((gemm_w8_kernel<G>), dim3(p.tiles_m * p.tiles_n, 1, splitk), dim3(G::T), 0, s, p);
}

}  // namespace

int gemm_w8_num_configs() { return quant_host::kNumCfg; }

int gemm_w8_max_splitk(int cfg, int K) {
  (void)cfg;
  return quant_host::max_splitk(K, BK);
}

void gemm_w8_pick(int M, int N, int K, int* cfg, int* splitk) {
  quant_host::pick(M, N, K, BK, 16, 8, cfg, splitk);
}

size_t gemm_w8_workspace_bytes(int M, int N, int splitk) {
  return quant_host::workspace_bytes(M, N, splitk);
}

void launch_gemm_w8(const GemmW8Args& a, hipStream_t s) {
  W8Params p{};
  p.A = (const bf16*)a.A;
  p.W = (const uint8_t*)a.Wq;
  p.scale = a.scale;
  p.C = (bf16*)a.C;
  p.bias = (const bf16*)a.bias;
  p.R = (const bf16*)a.R;
  p.lda = a.lda;
  p.ldw = a.ldw;
  p.ldc = a.ldc;
  p.ldr = a.ldr;
  p.M = a.M;
  p.N = a.N;
  p.K = a.K;
  p.act = a.act;
  p.alpha = a.alpha;
  p.pol = store_pol_aux((size_t)a.M * a.ldc * 2, a.store_pol);
  const quant_host::Split sp = quant_host::resolve_split(a.K, BK, a.splitk, a.workspace != nullptr);
  const int splitk = sp.splitk;
  p.kper = sp.kper;
  p.part = splitk > 1 ? a.workspace : nullptr;
  switch (a.config) {
    case 0: launch_cfg<W8C0>(p, splitk, s); break;
    case 1: launch_cfg<W8C1>(p, splitk, s); break;
    case 2: launch_cfg<W8C2>(p, splitk, s); break;
    default: launch_cfg<W8C3>(p, splitk, s); break;
  }
  if (splitk > 1) launch_quant_reduce<W8A16>(p, splitk, s);
}
