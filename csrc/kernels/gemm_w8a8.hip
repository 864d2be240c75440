// W8A8 GEMM on the block-scaled fp8 MFMA:
//   C = act(alpha * xscale[m] * scale[n] * sum_k Aq[m][k] * Wq[n][k] + bias[n]) + R
//
//   Aq [M][K] OCP e4m3 bytes (activation rows, K contiguous), xscale [M] fp32 (one per row)
//   Wq [N][K] OCP e4m3 bytes (weights, K contiguous), scale [N] fp32 (one per output channel)
//   C, R [M][N] bf16, bias [N] bf16; fp32 accumulation in the MFMA accumulators.
//
// Arithmetic: v_mfma_scale_f32_16x16x128_f8f6f4 with format 0 (e4m3) for both operands and
// NEUTRAL block scales (e8m0 code 127 = 2^0 in every scale byte, so whichever byte the
// instruction selects multiplies by exactly 1). The row and channel scales are applied once,
// in the epilogue. The instruction does four times the K of the bf16 16x16x32 MFMA in twice
// its cycles.
//
// Structure: the register-staged, double-buffered loop of gemm_w8.hip with BK = 128 BYTES for
// both operands: a row of a slice is 128 B in LDS (eight 16-byte chunks, chunk c of row r at
// c ^ (r & 7) as in gemm.hip). One barrier per K slice.
//
// K order inside a slice: the MFMA takes 32 bytes per lane and operand. Lane group g = lane >> 4
// reads bytes 32g .. 32g+31 of its row for BOTH operands (two ds_read_b128: chunks 2g, 2g+1),
// so whatever k map the instruction applies to a lane's 32 bytes, the same k of the activation
// row and of the weight row meet: a shared permutation of k leaves the sum unchanged.
//
// Operands are swapped (W is the MFMA's A operand) as in gemm_w8.hip: a lane's four accumulator
// values are four CONSECUTIVE output columns of one row, so the epilogue stores 8 bytes per
// fragment and a SwiGLU gate/up pair (weight rows interleaved in blocks of 16) is two fragments
// of one lane.
//
// K tails and out-of-range rows are zero-filled (code 0x00 is +0). K % 16 == 0.
//
// Split-K (grid.z): each split writes an fp32 partial slab, a second kernel sums the slabs in
// a fixed order and runs the epilogue — no atomics, bitwise reproducible.
#include "common.h"
#include "gemm_quant_host.h"
#include "gemm_quant_reduce.h"
#include "kernels.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;       // bytes (= e4m3 elements) of K per slice
constexpr int CH = BK / 16;   // 16-byte chunks per row of a slice
constexpr int kNeutral = 0x7f7f7f7f;  // e8m0 1.0 in every block-scale byte

template <int BM_, int BN_, int WAVES_M, int WAVES_N>
struct A8Cfg {
  static constexpr int BM = BM_, BN = BN_, WM = WAVES_M, WN = WAVES_N;
  static constexpr int T = 64 * WAVES_M * WAVES_N;
  static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  static constexpr int FM = WTM / 16, FN = WTN / 16;
  static constexpr int A_UNITS = BM * CH, W_UNITS = BN * CH;
  static constexpr int A_PER = (A_UNITS + T - 1) / T, W_PER = (W_UNITS + T - 1) / T;
  static constexpr int STAGE = A_UNITS + W_UNITS;  // 16-byte units per buffer
  static_assert(FM >= 1 && FN >= 2 && FN % 2 == 0, "wave tile: whole gate/up fragment pairs");
  static_assert(WTN % 32 == 0, "a wave's columns start on a gate/up block pair");
  static_assert(A_UNITS % T == 0 && W_UNITS % T == 0, "whole staging passes");
  static_assert(2 * STAGE * 16 <= 64 * 1024, "static LDS");
};

struct A8Params {
  const uint8_t* A;
  const uint8_t* W;
  const float* xscale;
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
struct W8A8 {
  using Params = A8Params;
  static constexpr bool kRowScale = true, kColScale = true;
};

template <class G>
__global__ __launch_bounds__(G::T) void gemm_w8a8_kernel(const A8Params p) {
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
      const int q = tid + i * G::T, row = q / CH, c = q % CH;
      const int gm = m0 + row, gk = k0 + c * 16;
      ra[i] = (gm < M && gk < kend) ? *reinterpret_cast<const u32x4*>(p.A + (size_t)gm * p.lda + gk) : zero4;
    }
#pragma unroll
    for (int i = 0; i < G::W_PER; ++i) {
      const int q = tid + i * G::T, row = q / CH, c = q % CH;
      const int gn = n0 + row, gk = k0 + c * 16;
      rw[i] = (gn < N && gk < kend) ? *reinterpret_cast<const u32x4*>(p.W + (size_t)gn * p.ldw + gk) : zero4;
    }
  };
  auto store_tile = [&](int buf) {
    u32x4* s = smem + buf * G::STAGE;
#pragma unroll
    for (int i = 0; i < G::A_PER; ++i) {
      const int q = tid + i * G::T, row = q / CH, c = q % CH;
      s[row * CH + (c ^ (row & 7))] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < G::W_PER; ++i) {
      const int q = tid + i * G::T, row = q / CH, c = q % CH;
      s[G::A_UNITS + row * CH + (c ^ (row & 7))] = rw[i];
    }
  };
  // bytes 32g .. 32g+31 of a staged row
  auto frag = [&](const u32x4* rows, int row) {
    const u32x4 lo = rows[row * CH + ((2 * g) ^ (row & 7))];
    const u32x4 hi = rows[row * CH + ((2 * g + 1) ^ (row & 7))];
    i32x8 f;
    f[0] = (int)lo[0]; f[1] = (int)lo[1]; f[2] = (int)lo[2]; f[3] = (int)lo[3];
    f[4] = (int)hi[0]; f[5] = (int)hi[1]; f[6] = (int)hi[2]; f[7] = (int)hi[3];
    return f;
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
    i32x8 af[G::FM], wf[G::FN];
#pragma unroll
    for (int i = 0; i < G::FM; ++i) af[i] = frag(s, wm * G::WTM + i * 16 + l16);
#pragma unroll
    for (int j = 0; j < G::FN; ++j) wf[j] = frag(s + G::A_UNITS, wn * G::WTN + j * 16 + l16);
#pragma unroll
    for (int i = 0; i < G::FM; ++i)
#pragma unroll
      for (int j = 0; j < G::FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 0, kNeutral, 0,
                                                                      kNeutral);
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
  float xs[G::FM];  // alpha * xscale of the lane's rows
#pragma unroll
  for (int i = 0; i < G::FM; ++i) {
    const int row = m0 + wm * G::WTM + i * 16 + l16;
    xs[i] = row < M ? p.alpha * p.xscale[row] : 0.f;
  }
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
        sg[e] = p.scale[gcol + e];
        su[e] = p.scale[gcol + 16 + e];
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
          float v = silu(xs[i] * sg[e] * acc[i][2 * jj][e] + bg[e]) * (xs[i] * su[e] * acc[i][2 * jj + 1][e] + bu[e]);
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
      sc[e] = in ? p.scale[col + e] : 0.f;
      bv[e] = (in && p.bias) ? bf2f(p.bias[col + e]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < G::FM; ++i) {
      const int row = m0 + wm * G::WTM + i * 16 + l16;
      if (row >= M) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = apply_act(xs[i] * sc[e] * acc[i][j][e] + bv[e], p.act);
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

using A8C0 = A8Cfg<128, 128, 2, 2>;
using A8C1 = A8Cfg<64, 128, 2, 2>;
using A8C2 = A8Cfg<64, 64, 2, 2>;
using A8C3 = A8Cfg<32, 64, 2, 2>;

template <class G>
void launch_cfg(A8Params p, int splitk, hipStream_t s) {
  p.tiles_m = (p.M + G::BM - 1) / G::BM;
  p.tiles_n = (p.N + G::BN - 1) / G::BN;
  hipLaunchKernelGGL((gemm_w8a8_kernel<G>), dim3(p.tiles_m * p.tiles_n, 1, splitk), dim3(G::T), 0, s, p);
}

}  // namespace

int gemm_w8a8_num_configs() { return quant_host::kNumCfg; }

int gemm_w8a8_max_splitk(int cfg, int K) {
  (void)cfg;
  return quant_host::max_splitk(K, BK);
}

void gemm_w8a8_pick(int M, int N, int K, int* cfg, int* splitk) {
  quant_host::pick(M, N, K, BK, 8, 4, cfg, splitk);
}

size_t gemm_w8a8_workspace_bytes(int M, int N, int splitk) {
  return quant_host::workspace_bytes(M, N, splitk);
}

void launch_gemm_w8a8(const GemmW8A8Args& a, hipStream_t s) {
  A8Params p{};
  p.A = (const uint8_t*)a.Aq;
  p.W = (const uint8_t*)a.Wq;
  p.xscale = a.xscale;
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
    case 0: launch_cfg<A8C0>(p, splitk, s); break;
    case 1: launch_cfg<A8C1>(p, splitk, s); break;
    case 2: launch_cfg<A8C2>(p, splitk, s); break;
    default: launch_cfg<A8C3>(p, splitk, s); break;
  }
  if (splitk > 1) launch_quant_reduce<W8A8>(p, splitk, s);
}
