// Grouped W8A16 GEMM (MoE experts with fp8 weights): G groups in ONE launch. Group g multiplies
// rows [offsets[g], offsets[g+1]) of A (or, with a_rows, the token rows a_rows[r]) by its own
// weight Wq_g (OCP e4m3 [N][K], address w_ptrs[g]) and channel scales (fp32 [N], s_ptrs[g]):
//
//   out[r][n] = act(scale_g[n] * sum_k A[row(r)][k] * Wq_g[n][k])
//
// written at the same rows of C, or compactly to rows 0..min(count, compact_rows)-1 of
// c_ptrs[g]. The contract of launch_gemm_glds_grouped with the arithmetic of gemm_w8.hip: every
// e4m3 value converts exactly to bf16 in registers, the bf16 MFMA accumulates in fp32, the scale
// is applied once in the epilogue. No split-K and no atomics: bitwise reproducible.
//
// Structure. The bf16 grouped kernel feeds both operands through LDS; here a tile's waves split
// its COLUMNS, so each weight byte is needed by exactly one wave and goes global -> VGPR
// directly, in the operand layout gemm_w8.hip reads from LDS: lane (l16, g = lane >> 4) holds
// k = 16g .. 16g+15 of weight row l16 of a 16-row fragment, one 16-byte load per fragment and
// 64-wide K slice, feeding two 16x16x32 MFMA steps. The loads run several slices ahead in a
// register ring. Only the (gathered) activation rows go through LDS: 128-byte rows, chunk c of
// row r at c ^ (r & 7), register-staged (a ring, too) and double buffered, one barrier per
// slice; every wave reads the whole row tile. A block owns (group, column tile) and walks the
// group's row tiles, so a group of any count is valid: zero rows exit, a partial tile computes
// rows it never stores, a tall group takes passes (re-reading its weight panel; the tall configs
// cover a typical expert in one).
//
// Operands are swapped as in gemm_w8.hip (W is the MFMA's A operand): a lane's four accumulator
// values are four consecutive output columns of one row, and a SwiGLU gate/up pair (weight rows
// interleaved in blocks of 16) is two fragments of one lane.
#include "common.h"
#include "kernels.h"

namespace {

// the weights' addresses come from a device array: without the global address space on the load
// the compiler emits FLAT loads, which also count as LDS traffic — every wait for an LDS read
// would then wait for the whole weight ring
typedef const __attribute__((address_space(1))) u32x4 global_u32x4;

constexpr int BK = 64;
constexpr int ACH = BK / 8;  // 16-byte chunks per A row of a slice

// PF: weight slices held in the register ring (the current one included: loads run PF - 1 slices
// ahead); AD: activation slices in the staging ring (a slice is loaded AD - 1 iterations before
// its LDS store). One block's MFMAs per slice are far shorter than the memory latency, so both
// rings — and the blocks sharing a CU — are what keeps bytes in flight.
// OCC: waves per SIMD the register budget is held to (2: two 4-wave blocks share a CU).
template <int BM_, int WTN_, int WAVES_, int PF_, int AD_, int OCC_ = 1>
struct GW8Cfg {
  static constexpr int BM = BM_, WTN = WTN_, WAVES = WAVES_, PF = PF_, AD = AD_, OCC = OCC_;
  static constexpr int BN = WTN * WAVES, T = 64 * WAVES;
  static constexpr int FM = BM / 16, FN = WTN / 16;
  static constexpr int A_UNITS = BM * ACH;
  static constexpr int A_PER = (A_UNITS + T - 1) / T;
  static_assert(BM % 16 == 0 && WTN % 32 == 0, "whole fragments; a wave's columns are gate/up block pairs");
  static_assert(A_UNITS % T == 0 && T % ACH == 0, "every thread stages whole chunks of fixed rows");
  static_assert(2 * A_UNITS * 16 <= 64 * 1024, "static LDS");
  static_assert(PF >= 2 && AD >= 2 && PF % AD == 0 && PF % 2 == 0, "the K loop is unrolled PF times: static slots");
};

struct GW8Params {
  const bf16* A;
  int lda;
  const int* a_rows;  // or nullptr
  const int* offsets;
  const unsigned long long* w_ptrs;
  const unsigned long long* s_ptrs;
  const unsigned long long* c_ptrs;  // compact outputs, or nullptr
  bf16* C;
  int ldc;
  int R, N, K;
  int act;
  int compact_rows;
  int groups, tiles_n;
  int shared;  // same-weight groups are adjacent: run a column tile's groups side by side
  int pol;
};

template <class G>
__global__ __launch_bounds__(G::T, G::OCC) void gemm_w8_grouped_kernel(const GW8Params p) {
  __shared__ u32x4 smem[2 * G::A_UNITS];
  constexpr int BM = G::BM, FM = G::FM, FN = G::FN, PF = G::PF, AD = G::AD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  int grp, tn;
  if (p.shared) {
    grp = blockIdx.x % p.groups;
    tn = blockIdx.x / p.groups;
  } else {
    grp = blockIdx.x / p.tiles_n;
    tn = blockIdx.x % p.tiles_n;
  }
  const int r0 = max(p.offsets[grp], 0), r1 = min(p.offsets[grp + 1], p.R);
  const int count = r1 - r0;
  if (count <= 0) return;
  const int N = p.N, K = p.K;
  const unsigned long long W = p.w_ptrs[grp];
  const float* __restrict__ scale = reinterpret_cast<const float*>(p.s_ptrs[grp]);
  const int wn0 = tn * G::BN + wave * G::WTN;  // this wave's first weight row (output column)
  const int nk = (K + BK - 1) / BK;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // this lane's 16 bytes of every weight fragment: row wn0 + 16j + l16, k = 64 kt + 16 g ..
  // Every load is UNCONDITIONAL at a clamped (valid) address, and what must be zero (k past K:
  // the last slice's tail, ring slots past the end) is zeroed by a select where the value is
  // CONSUMED, slices later: a load under a divergent branch, or a select right behind the load,
  // makes the wave wait for the load at once, and the register rings would prefetch nothing.
  // Weight rows past N are clamped, not zeroed: they only feed output columns never stored.
  unsigned long long wp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = W + (unsigned long long)min(wn0 + j * 16 + l16, N - 1) * K;
  auto load_w = [&](int kt, u32x4(&dst)[FN]) {
    const int ko = min(kt * BK + 16 * g, K - 16);
#pragma unroll
    for (int j = 0; j < FN; ++j) dst[j] = *reinterpret_cast<global_u32x4*>(wp[j] + ko);
  };

  bf16* Cg;
  int out_rows, crow0;  // rows of this group that are written, first output row
  if (p.c_ptrs != nullptr) {
    Cg = reinterpret_cast<bf16*>(p.c_ptrs[grp]);
    out_rows = min(count, p.compact_rows);
    crow0 = 0;
  } else {
    Cg = p.C;
    out_rows = count;
    crow0 = r0;
  }
  const int ldc = p.ldc;
  const bool vec_ok = (ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(Cg) & 7) == 0);
  const int a_chunk = tid % ACH, a_row = tid / ACH;  // unit q = tid + i*T: row a_row + i*(T/ACH), same chunk

  for (int m0 = 0; m0 < out_rows; m0 += BM) {
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // source row of every A unit this thread stages; tile rows past the group's count read its
    // last row (their output rows are never stored)
    const bf16* ap[G::A_PER];
#pragma unroll
    for (int i = 0; i < G::A_PER; ++i) {
      const int m = min(m0 + a_row + i * (G::T / ACH), count - 1);
      const int src = p.a_rows ? p.a_rows[r0 + m] : r0 + m;
      ap[i] = p.A + (size_t)src * p.lda;
    }
    // slice k of A waits in ring slot k % AD between its load and its LDS store
    u32x4 ra[AD][G::A_PER];
    auto load_a = [&](int kt, u32x4(&dst)[G::A_PER]) {
      const int ko = min(kt * BK + a_chunk * 8, K - 8);
#pragma unroll
      for (int i = 0; i < G::A_PER; ++i) dst[i] = *reinterpret_cast<const u32x4*>(ap[i] + ko);
    };
    auto store_a = [&](int kt, const u32x4(&src)[G::A_PER]) {  // slice kt -> LDS buffer kt & 1
      u32x4* s = smem + (kt & 1) * G::A_UNITS;
      const bool in = kt * BK + a_chunk * 8 < K;
#pragma unroll
      for (int i = 0; i < G::A_PER; ++i) {
        const int row = a_row + i * (G::T / ACH);
        s[row * ACH + (a_chunk ^ (row & 7))] = in ? src[i] : zero4;
      }
    };

    u32x4 wr[PF][FN];
    load_a(0, ra[0]);
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      load_w(s, wr[s]);
      if (s >= 1 && s < AD) load_a(s, ra[s]);
    }
    store_a(0, ra[0]);
    __syncthreads();
    // Straight-line body, unrolled PF times (PF even: ring slots and the LDS buffer are static),
    // over K padded to whole groups of PF slices: a slice past K loads zeros and adds nothing.
    // No branch inside, so the compiler counts the loads in flight exactly at every wait.
    for (int kt0 = 0; kt0 < nk; kt0 += PF) {
#pragma unroll
      for (int s = 0; s < PF; ++s) {
        const int kt = kt0 + s;
        load_a(kt + AD, ra[s % AD]);  // into the slot of slice kt, which is in LDS already
        u32x4 w[FN];
        const bool w_in = kt * BK + 16 * g < K;
#pragma unroll
        for (int j = 0; j < FN; ++j) w[j] = w_in ? wr[s][j] : zero4;
        load_w(kt + PF, wr[s]);  // refill the ring slot: PF slices ahead
        const u32x4* sm = smem + (s & 1) * G::A_UNITS;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          bf16x8 wf[FN];
#pragma unroll
          for (int j = 0; j < FN; ++j) wf[j] = cvt_e4m3x8(w[j][2 * h], w[j][2 * h + 1]);
          // LDS reads in batches ahead of their MFMAs: one read, one wait, two MFMAs in turn
          // would expose the LDS latency FM times per step with a single wave per SIMD
          constexpr int AB = FM < 8 ? FM : 8;
#pragma unroll
          for (int i0 = 0; i0 < FM; i0 += AB) {
            u32x4 av[AB];
#pragma unroll
            for (int i = 0; i < AB; ++i) {
              const int row = (i0 + i) * 16 + l16;
              av[i] = sm[row * ACH + ((2 * g + h) ^ (row & 7))];
            }
#pragma unroll
            for (int i = 0; i < AB; ++i) {
              const bf16x8 af = *reinterpret_cast<const bf16x8*>(&av[i]);
#pragma unroll
              for (int j = 0; j < FN; ++j) acc[i0 + i][j] = mfma16x16x32(wf[j], af, acc[i0 + i][j]);
            }
          }
        }
        store_a(kt + 1, ra[(s + 1) % AD]);
        __syncthreads();
      }
    }

    // lane: tile row i*16 + l16, columns wn0 + j*16 + 4g .. +3
    if (p.act == ACT_SWIGLU) {
      // fragments (2jj, 2jj+1) of a lane: gate and up of the same four output columns
      const int NO = N / 2;
#pragma unroll
      for (int jj = 0; jj < FN / 2; ++jj) {
        const int gcol = wn0 + jj * 32 + 4 * g;
        const int ocol = wn0 / 2 + jj * 16 + 4 * g;
        if (ocol >= NO) continue;  // N % 32 == 0: a block pair is inside N or past it as a whole
        float sg[4], su[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sg[e] = scale[gcol + e];
          su[e] = scale[gcol + 16 + e];
        }
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int m = m0 + i * 16 + l16;
          if (m >= out_rows) continue;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(silu(sg[e] * acc[i][2 * jj][e]) * (su[e] * acc[i][2 * jj + 1][e]));
          const size_t idx = (size_t)(crow0 + m) * ldc + ocol;
          if (vec_ok) {
            store_bf16x4(Cg, idx, o, p.pol);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) Cg[idx + e] = o[e];
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = wn0 + j * 16 + 4 * g;
        if (col >= N) continue;
        float sc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[e] = col + e < N ? scale[col + e] : 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int m = m0 + i * 16 + l16;
          if (m >= out_rows) continue;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(apply_act(sc[e] * acc[i][j][e], p.act));
          const size_t idx = (size_t)(crow0 + m) * ldc + col;
          if (vec_ok && col + 3 < N) {
            store_bf16x4(Cg, idx, o, p.pol);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < N) Cg[idx + e] = o[e];
          }
        }
      }
    }
  }
}

using GW8C0 = GW8Cfg<32, 32, 4, 8, 4, 2>;    // short: small counts (few rows per expert)
using GW8C1 = GW8Cfg<128, 32, 4, 8, 2>;      // 128 rows x 128 columns, one block per CU, deep weight ring
using GW8C2 = GW8Cfg<128, 32, 8, 4, 2, 2>;   // 128 rows x 256 columns over 8 waves: one A tile feeds twice the columns
using GW8C3 = GW8Cfg<192, 32, 4, 8, 2>;      // 192 rows: the expected Mixtral expert (128 rows at M = 512) and
                                             // most of the busiest ones (149-227) in one pass over the weight panel
using GW8C4 = GW8Cfg<192, 32, 8, 4, 2, 2>;   // the same over 8 waves and 256 columns
constexpr int kNumCfg = 5;
constexpr int kTileRows[kNumCfg] = {GW8C0::BM, GW8C1::BM, GW8C2::BM, GW8C3::BM, GW8C4::BM};

template <class G>
void launch_cfg(GW8Params p, hipStream_t s) {
  p.tiles_n = (p.N + G::BN - 1) / G::BN;
  hipLaunchKernelGGL((gemm_w8_grouped_kernel<G>), dim3(p.groups * p.tiles_n), dim3(G::T), 0, s, p);
}

}  // namespace

int gemm_w8_grouped_num_configs() { return kNumCfg; }

int gemm_w8_grouped_tile_rows(int cfg) { return kTileRows[cfg < 0 || cfg >= kNumCfg ? 0 : cfg]; }

int gemm_w8_grouped_pick(int rows_hint, int N, int K, int n_groups) {
  // Fitted to the cold-weight measurements of Mixtral's expert GEMMs (benchmarks/bench_grouped_w8.py,
  // profiles/w8_experts/grouped_w8.txt). A block re-reads its weight panel once per row tile of its
  // group and the launch ends with its slowest block, so the tile height goes by the BUSIEST group
  // to expect, about 1.5 x the mean (rows_hint): the short tile for a handful of rows, 128 rows up
  // to a mean of 96, 192 rows beyond (a 256-row tile's 128 accumulator registers per lane made it
  // slower than two passes of 192). Columns: 256 over 8 waves when that still gives two rounds of
  // blocks on the 256 CUs (gate/up), else 128 over 4 waves (down: 256 blocks, long K).
  (void)K;
  if (rows_hint <= 32) return 0;
  const bool wide = (long)n_groups * ((N + 255) / 256) >= 512;
  if (rows_hint <= 96) return wide ? 2 : 1;
  return wide ? 4 : 3;
}

void launch_gemm_w8_grouped(const GemmW8GroupedArgs& a, hipStream_t s) {
  if (a.n_groups <= 0 || a.R <= 0 || a.N <= 0) return;
  GW8Params p{};
  p.A = (const bf16*)a.A;
  p.lda = a.lda;
  p.a_rows = a.a_rows;
  p.offsets = a.offsets;
  p.w_ptrs = a.w_ptrs;
  p.s_ptrs = a.s_ptrs;
  p.c_ptrs = a.c_ptrs;
  p.C = (bf16*)a.C;
  p.ldc = a.ldc;
  p.R = a.R;
  p.N = a.N;
  p.K = a.K;
  p.act = a.act;
  p.compact_rows = a.compact_rows;
  p.groups = a.n_groups;
  p.shared = a.shared_weights;
  const size_t out_rows = a.c_ptrs != nullptr ? (size_t)a.compact_rows : (size_t)a.R;
  p.pol = store_pol_aux(out_rows * a.ldc * 2, a.store_pol);
  switch (a.config) {
    case 0: launch_cfg<GW8C0>(p, s); break;
    case 1: launch_cfg<GW8C1>(p, s); break;
    case 2: launch_cfg<GW8C2>(p, s); break;
    case 3: launch_cfg<GW8C3>(p, s); break;
    default: launch_cfg<GW8C4>(p, s); break;
  }
}
