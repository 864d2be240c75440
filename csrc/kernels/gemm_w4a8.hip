// W4A8 GEMM on the block-scaled MFMA with MXFP4 weights:
//   C = act(alpha * xscale[m] * sum_k Aq[m][k] * W[n][k] + bias[n]) + R
//
//   Aq [M][K] OCP e4m3 bytes (activation rows, K contiguous), xscale [M] fp32 (one per row)
//   W  [N][K] OCP MXFP4: Wq [N][K/2] bytes, element k of a row in the low (k even) / high (k odd)
//      nibble of byte k/2 (e2m1), and Ws [N][K/32] e8m0 bytes, W[n][k] = e2m1 * 2^(Ws[n][k/32] - 127)
//   C, R [M][N] bf16, bias [N] bf16; fp32 accumulation in the MFMA accumulators.
//
// Arithmetic: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4 (first operand e2m1 in four VGPRs,
// the upper four of the i32x8 zero) and blgp = 0 (second operand e4m3). The activation side keeps
// the neutral block scale 0x7f7f7f7f; the weight side carries the stored e8m0 code of the lane's
// block, so the hardware dequantises: no conversion instruction runs. The row scale is applied
// once, in the epilogue.
//
// Lane maps (benchmarks/mfma_fp4_probe.hip, measured): an fp4 lane (l16, g = lane >> 4) holds row
// l16, k = 32g + e for element e of its 32, element e the low / high nibble of byte e / 2 of its
// 16 bytes, i.e. the stored order; its own scale register scales those 32 elements and op_sel j
// selects byte j of it. An e4m3 lane (l16, g) does NOT hold 32 consecutive k: bytes 0..15 are
// k = 16g .. 16g+15 and bytes 16..31 are k = 64 + 16g .. 64 + 16g+15. So lane group g reads bytes
// 16g .. 16g+15 of a weight row's 64-byte slice (one ds_read_b128), the scale byte
// Ws[n][4 * slice + g], and the 16-byte chunks g and 4 + g of the activation row's 128-byte slice:
// the order is fixed where the fragments are read, the stored formats are untouched.
//
// Structure: the register-staged, double-buffered loop of gemm_w8a8.hip with BK = 128 elements:
// an activation row of a slice is 128 B in LDS (eight 16-byte chunks, chunk c of row r at
// c ^ (r & 7)), a weight row 64 B (four chunks, chunk c of row r at c ^ ((r >> 1) & 3): two rows
// span the 128 B the xor of gemm.hip covers) plus one dword of four scale bytes. One barrier per
// K slice.
//
// Operands are swapped (W is the MFMA's first operand) as in gemm_w8a8.hip: a lane's four
// accumulator values are four CONSECUTIVE output columns of one row, so the epilogue stores 8
// bytes per fragment and a SwiGLU gate/up pair (weight rows interleaved in blocks of 16) is two
// fragments of one lane.
//
// K tails and out-of-range rows are zero-filled with scale code 127 (a zero times 2^0; any
// other fill could meet code 255, NaN). K % 32 == 0: whole blocks. Any scale code 0..254.
//
// Split-K (grid.z): each split writes an fp32 partial slab, a second kernel sums the slabs in
// a fixed order and runs the epilogue — no atomics, bitwise reproducible.
#include "common.h"
#include "gemm_quant_host.h"
#include "gemm_quant_reduce.h"
#include "kernels.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;       // elements of K per slice
constexpr int CH = BK / 16;   // 16-byte chunks per activation row of a slice (e4m3: 128 B)
constexpr int CW = BK / 32;   // 16-byte chunks per weight row of a slice (e2m1: 64 B) = blocks
constexpr int kNeutral = 0x7f7f7f7f;  // e8m0 1.0 in every block-scale byte

template <int BM_, int BN_, int WAVES_M, int WAVES_N>
struct W4Cfg {
  static constexpr int BM = BM_, BN = BN_, WM = WAVES_M, WN = WAVES_N;
  static constexpr int T = 64 * WAVES_M * WAVES_N;
  static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  static constexpr int FM = WTM / 16, FN = WTN / 16;
  static constexpr int A_UNITS = BM * CH, W_UNITS = BN * CW, S_UNITS = BN / 4;  // scales: a dword per row
  static constexpr int A_PER = (A_UNITS + T - 1) / T, W_PER = (W_UNITS + T - 1) / T;
  static constexpr int STAGE = A_UNITS + W_UNITS + S_UNITS;  // 16-byte units per buffer
  static_assert(FM >= 1 && FN >= 2 && FN % 2 == 0, "wave tile: whole gate/up fragment pairs");
  static_assert(WTN % 32 == 0, "a wave's columns start on a gate/up block pair");
  static_assert(A_UNITS % T == 0 && W_UNITS % T == 0, "whole staging passes");
  static_assert(BN <= T && BN % 4 == 0, "one thread stages a row's scale dword");
  static_assert(2 * STAGE * 16 <= 64 * 1024, "static LDS");
};

struct W4Params {
  const uint8_t* A;
  const uint8_t* W;  // e2m1 pairs [N][ldw bytes]
  const uint8_t* S;  // e8m0 [N][lds]
  const float* xscale;
  bf16* C;
  const bf16* bias;
  const bf16* R;
  float* part;  // split-K: fp32 [splitk][M][N]
  int lda, ldw, lds, ldc, ldr;
  int s_dword;  // scale rows and base 4-byte aligned: a slice's four codes are one load
  int M, N, K;
  int act;
  float alpha;
  int tiles_m, tiles_n;
  int kper;  // K elements per split (a multiple of BK)
  int pol;   // store8_pol aux bits of the output stores (0, 2 nt, 16 write-through)
};

// the format to gemm_quant_reduce.h
struct W4A8 {
  using Params = W4Params;
  static constexpr bool kRowScale = true, kColScale = false;
};

template <class G>
__global__ __launch_bounds__(G::T) void gemm_w4a8_kernel(const W4Params p) {
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
  uint32_t rs = kNeutral;  // thread tid < BN: the four scale codes of weight row tid in the slice
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
      const int q = tid + i * G::T, row = q / CW, c = q % CW;
      const int gn = n0 + row, gk = k0 + c * 32;  // chunk c: block c of the slice, 16 bytes
      rw[i] = (gn < N && gk < kend) ? *reinterpret_cast<const u32x4*>(p.W + (size_t)gn * p.ldw + gk / 2) : zero4;
    }
    if (tid < BN) {
      const int gn = n0 + tid, nb = (kend - k0) / 32;  // blocks of the slice inside K (kend % 32 == 0)
      rs = kNeutral;
      if (gn < N) {
        const uint8_t* sp = p.S + (size_t)gn * p.lds + k0 / 32;
        if (p.s_dword && nb >= CW) {
          rs = *reinterpret_cast<const uint32_t*>(sp);
        } else {
#pragma unroll
          for (int j = 0; j < CW; ++j)
            if (j < nb) rs = (rs & ~(0xffu << (8 * j))) | ((uint32_t)sp[j] << (8 * j));
        }
      }
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
      const int q = tid + i * G::T, row = q / CW, c = q % CW;
      s[G::A_UNITS + row * CW + (c ^ ((row >> 1) & 3))] = rw[i];
    }
    if (tid < BN) reinterpret_cast<uint32_t*>(s + G::A_UNITS + G::W_UNITS)[tid] = rs;
  };
  // bytes 16g .. 16g+15 and 64 + 16g .. 64 + 16g+15 of a staged activation row (the e4m3 k map)
  auto frag = [&](const u32x4* rows, int row) {
    const u32x4 lo = rows[row * CH + (g ^ (row & 7))];
    const u32x4 hi = rows[row * CH + ((4 + g) ^ (row & 7))];
    i32x8 f;
    f[0] = (int)lo[0]; f[1] = (int)lo[1]; f[2] = (int)lo[2]; f[3] = (int)lo[3];
    f[4] = (int)hi[0]; f[5] = (int)hi[1]; f[6] = (int)hi[2]; f[7] = (int)hi[3];
    return f;
  };
  // bytes 16g .. 16g+15 of a staged weight row: elements 32g .. 32g+31 in the stored nibble order
  auto wfrag = [&](const u32x4* rows, int row) {
    const u32x4 v = rows[row * CW + (g ^ ((row >> 1) & 3))];
    i32x8 f = {(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
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
    int ws[G::FN];  // e8m0 code of the lane's block in byte 0
#pragma unroll
    for (int i = 0; i < G::FM; ++i) af[i] = frag(s, wm * G::WTM + i * 16 + l16);
#pragma unroll
    for (int j = 0; j < G::FN; ++j) {
      const int row = wn * G::WTN + j * 16 + l16;
      wf[j] = wfrag(s + G::A_UNITS, row);
      ws[j] = reinterpret_cast<const uint8_t*>(s + G::A_UNITS + G::W_UNITS)[row * 4 + g];
    }
#pragma unroll
    for (int i = 0; i < G::FM; ++i)
#pragma unroll
      for (int j = 0; j < G::FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[i][j], 4, 0, 0, ws[j], 0,
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
      float bg[4], bu[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
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
          float v = silu(xs[i] * acc[i][2 * jj][e] + bg[e]) * (xs[i] * acc[i][2 * jj + 1][e] + bu[e]);
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
    float bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = col + e < N;
      bv[e] = (in && p.bias) ? bf2f(p.bias[col + e]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < G::FM; ++i) {
      const int row = m0 + wm * G::WTM + i * 16 + l16;
      if (row >= M) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = apply_act(xs[i] * acc[i][j][e] + bv[e], p.act);
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

using W4C0 = W4Cfg<128, 128, 2, 2>;
using W4C1 = W4Cfg<64, 128, 2, 2>;
using W4C2 = W4Cfg<64, 64, 2, 2>;
using W4C3 = W4Cfg<32, 64, 2, 2>;

template <class G>
void launch_cfg(W4Params p, int splitk, hipStream_t s) {
  p.tiles_m = (p.M + G::BM - 1) / G::BM;
  p.tiles_n = (p.N + G::BN - 1) / G::BN;
  hipLaunchKernelGGL((gemm_w4a8_kernel<G>), dim3(p.tiles_m * p.tiles_n, 1, splitk), dim3(G::T), 0, s, p);
}

}  // namespace

int gemm_w4a8_num_configs() { return quant_host::kNumCfg; }

int gemm_w4a8_max_splitk(int cfg, int K) {
  (void)cfg;
  return quant_host::max_splitk(K, BK);
}

void gemm_w4a8_pick(int M, int N, int K, int* cfg, int* splitk) {
  quant_host::pick(M, N, K, BK, 8, 4, cfg, splitk);
}

size_t gemm_w4a8_workspace_bytes(int M, int N, int splitk) {
  return quant_host::workspace_bytes(M, N, splitk);
}

void launch_gemm_w4a8(const GemmW4A8Args& a, hipStream_t s) {
  W4Params p{};
  p.A = (const uint8_t*)a.Aq;
  p.W = (const uint8_t*)a.Wq;
  p.S = (const uint8_t*)a.Ws;
  p.xscale = a.xscale;
  p.C = (bf16*)a.C;
  p.bias = (const bf16*)a.bias;
  p.R = (const bf16*)a.R;
  p.lda = a.lda;
  p.ldw = a.ldw;
  p.lds = a.lds;
  p.s_dword = a.lds % 4 == 0 && (reinterpret_cast<uintptr_t>(a.Ws) & 3) == 0;
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
    case 0: launch_cfg<W4C0>(p, splitk, s); break;
    case 1: launch_cfg<W4C1>(p, splitk, s); break;
    case 2: launch_cfg<W4C2>(p, splitk, s); break;
    default: launch_cfg<W4C3>(p, splitk, s); break;
  }
  if (splitk > 1) launch_quant_reduce<W4A8>(p, splitk, s);
}
