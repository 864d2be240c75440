// Grouped W4A8 GEMM (MoE experts with MXFP4 weights): G groups in ONE launch. Group g multiplies
// the sorted rows [offsets[g], offsets[g+1]) — row r of Aq, or the token row a_rows[r] of Aq —
// by its own weight W_g (OCP MXFP4: e2m1 pairs [N][K/2] at w_ptrs[g], e8m0 block scales
// [N][K/32] at s_ptrs[g], any code 0..254):
//
//   out[r][n] = act(xscale[row(r)] * sum_k Aq[row(r)][k] * W_g[n][k]),  row(r) = a_rows ? a_rows[r] : r
//
// Aq is e4m3 with one fp32 scale per SOURCE row: with a_rows the scale of sorted row r is
// xscale[a_rows[r]], not xscale[r]. Output bf16 at the same rows of C, or compactly to rows
// 0..min(count, compact_rows)-1 of c_ptrs[g]. The contract of launch_gemm_w8_grouped with the
// arithmetic of gemm_w4a8.hip: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4 (first operand
// e2m1 in four VGPRs), the weight side carrying the stored e8m0 code of the lane's block, the
// activation side the neutral code; no conversion instruction runs. The row scale is applied once,
// in the epilogue. No split-K and no atomics: bitwise reproducible.
//
// Structure: that of gemm_w8_grouped.hip with BK = 128 elements. A tile's waves split its
// COLUMNS, so each weight byte is needed by exactly one wave and goes global -> VGPR directly in
// the operand layout (lane maps: benchmarks/mfma_fp4_probe.hip): an fp4 lane (l16, g = lane >> 4)
// holds k = 32g .. 32g+31 of weight row l16, which are bytes 16g .. 16g+15 of the row's 64-byte
// slice in stored order — one 16-byte load per fragment and slice, straight into the MFMA. The
// lane's block-scale code is Ws[n][4 * slice + g]: with 4-byte aligned scale rows (K % 128 == 0,
// aligned base) the slice's dword is loaded and shifted by 8g (op_sel is an immediate and cannot
// vary by lane), otherwise one byte is loaded. Both run several slices ahead in a register ring.
// Only the (gathered) e4m3 activation rows go through LDS: 128-byte rows per slice, chunk c of
// row r at c ^ (r & 7), register-staged (a ring, too) and double buffered, one barrier per slice;
// lane group g reads the 16-byte chunks g and 4 + g (the e4m3 k map of gemm_w4a8.hip: bytes
// 0..15 of an e4m3 lane are k = 16g.., bytes 16..31 are k = 64 + 16g..). A block owns (group,
// column tile) and walks the group's row tiles: zero rows exit, a partial tile computes rows it
// never stores, a tall group takes passes (one config picks a taller tile for such a group).
//
// The three rules of gemm_w8_grouped.hip hold here: loads are unconditional at clamped addresses
// inside the tensor and zeroing is a select where the value is consumed; addresses read from the
// pointer arrays are dereferenced through the global address space (no FLAT loads); the K loop is
// branch-free over K padded to whole ring turns. A zeroed data chunk times any code 0..254 is
// zero, so only the data takes the select (the clamped scale loads stay inside the tensor and so
// never meet code 255). K % 32 == 0: K tails are whole blocks.
//
// Operands are swapped (W is the MFMA's first operand): a lane's four accumulator values are four
// consecutive output columns of one row, and a SwiGLU gate/up pair (rows of q and s interleaved in
// blocks of 16) is two fragments of one lane.
#include "common.h"
#include "kernels.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) u32x4 global_u32x4;
typedef const __attribute__((address_space(1))) uint32_t global_u32;
typedef const __attribute__((address_space(1))) uint8_t global_u8;

constexpr int BK = 128;      // elements of K per slice
constexpr int ACH = BK / 16;  // 16-byte chunks per activation row of a slice (e4m3: 128 B)
constexpr int kNeutral = 0x7f7f7f7f;  // e8m0 1.0 in every block-scale byte

// PF: weight (and scale) slices in the register ring, the current one included; AD: activation
// slices in the staging ring; OCC: waves per SIMD the register budget is held to.
template <int BM_, int WTN_, int WAVES_, int PF_, int AD_, int OCC_ = 1>
struct GW4Cfg {
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

struct GW4Params {
  const uint8_t* A;  // e4m3 [.][lda bytes]
  int lda;
  const float* xscale;  // fp32, one per SOURCE row of A
  const int* a_rows;    // or nullptr
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

// SDW: the scale rows are 4-byte aligned (K % 128 == 0 and every base aligned): a slice's four
// codes are one dword load; else one byte load per lane. A template parameter, not a branch:
// the K loop stays straight-line.
// One (group, column tile) with row tiles of G::BM rows: the whole K loop and the epilogue.
template <class G, bool SDW>
__device__ __forceinline__ void gw4_group(const GW4Params& p, u32x4* smem, int grp, int tn, int r0, int count) {
  constexpr int BM = G::BM, FM = G::FM, FN = G::FN, PF = G::PF, AD = G::AD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int N = p.N, K = p.K;
  const int KB = K / 2, KS = K / 32;  // bytes of a weight row, of a scale row
  const unsigned long long W = p.w_ptrs[grp], S = p.s_ptrs[grp];
  const int wn0 = tn * G::BN + wave * G::WTN;  // this wave's first weight row (output column)
  const int nk = (K + BK - 1) / BK;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // this lane's 16 bytes of every weight fragment: row wn0 + 16j + l16, bytes 64 kt + 16 g ..,
  // and its block's code, byte 4 kt + g of the row's scales. Every load is UNCONDITIONAL at a
  // clamped (valid) address; what must be zero (k past K: the last slice's tail, ring slots past
  // the end) is zeroed by a select where the value is CONSUMED, slices later. Weight rows past N
  // are clamped, not zeroed: they only feed output columns never stored.
  unsigned long long wp[FN], sp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const unsigned long long row = (unsigned long long)min(wn0 + j * 16 + l16, N - 1);
    wp[j] = W + row * KB;
    sp[j] = S + row * KS;
  }
  auto load_w = [&](int kt, u32x4(&dst)[FN], uint32_t(&sc)[FN]) {
    const int ko = min(kt * (BK / 2) + 16 * g, KB - 16);
    const int so = SDW ? 4 * min(kt, nk - 1) : min(4 * kt + g, KS - 1);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      dst[j] = *reinterpret_cast<global_u32x4*>(wp[j] + ko);
      if constexpr (SDW) sc[j] = *reinterpret_cast<global_u32*>(sp[j] + so);
      else sc[j] = *reinterpret_cast<global_u8*>(sp[j] + so);
    }
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
    const uint8_t* ap[G::A_PER];
#pragma unroll
    for (int i = 0; i < G::A_PER; ++i) {
      const int m = min(m0 + a_row + i * (G::T / ACH), count - 1);
      const int src = p.a_rows ? p.a_rows[r0 + m] : r0 + m;
      ap[i] = p.A + (size_t)src * p.lda;
    }
    // slice k of A waits in ring slot k % AD between its load and its LDS store
    u32x4 ra[AD][G::A_PER];
    auto load_a = [&](int kt, u32x4(&dst)[G::A_PER]) {
      const int ko = min(kt * BK + a_chunk * 16, K - 16);
#pragma unroll
      for (int i = 0; i < G::A_PER; ++i) dst[i] = *reinterpret_cast<const u32x4*>(ap[i] + ko);
    };
    auto store_a = [&](int kt, const u32x4(&src)[G::A_PER]) {  // slice kt -> LDS buffer kt & 1
      u32x4* s = smem + (kt & 1) * G::A_UNITS;
      const bool in = kt * BK + a_chunk * 16 < K;
#pragma unroll
      for (int i = 0; i < G::A_PER; ++i) {
        const int row = a_row + i * (G::T / ACH);
        s[row * ACH + (a_chunk ^ (row & 7))] = in ? src[i] : zero4;
      }
    };

    u32x4 wr[PF][FN];
    uint32_t sr[PF][FN];
    load_a(0, ra[0]);
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      load_w(s, wr[s], sr[s]);
      if (s >= 1 && s < AD) load_a(s, ra[s]);
    }
    store_a(0, ra[0]);
    __syncthreads();
    // Straight-line body, unrolled PF times (PF even: ring slots and the LDS buffer are static),
    // over K padded to whole groups of PF slices: a slice past K multiplies zeros and adds nothing.
    for (int kt0 = 0; kt0 < nk; kt0 += PF) {
#pragma unroll
      for (int s = 0; s < PF; ++s) {
        const int kt = kt0 + s;
        load_a(kt + AD, ra[s % AD]);  // into the slot of slice kt, which is in LDS already
        i32x8 wf[FN];
        int ws[FN];  // e8m0 code of the lane's block in byte 0
        const bool w_in = kt * BK + 32 * g < K;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const u32x4 w = w_in ? wr[s][j] : zero4;
          wf[j] = i32x8{(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
          ws[j] = SDW ? (int)((sr[s][j] >> (8 * g)) & 0xffu) : (int)sr[s][j];
        }
        load_w(kt + PF, wr[s], sr[s]);  // refill the ring slot: PF slices ahead
        const u32x4* sm = smem + (s & 1) * G::A_UNITS;
        // LDS reads in batches ahead of their MFMAs (two 16-byte reads per fragment)
        constexpr int AB = FM < 4 ? FM : 4;
#pragma unroll
        for (int i0 = 0; i0 < FM; i0 += AB) {
          u32x4 lo[AB], hi[AB];
#pragma unroll
          for (int i = 0; i < AB; ++i) {
            const int row = (i0 + i) * 16 + l16;
            lo[i] = sm[row * ACH + (g ^ (row & 7))];
            hi[i] = sm[row * ACH + ((4 + g) ^ (row & 7))];
          }
#pragma unroll
          for (int i = 0; i < AB; ++i) {
            const i32x8 af = {(int)lo[i][0], (int)lo[i][1], (int)lo[i][2], (int)lo[i][3],
                              (int)hi[i][0], (int)hi[i][1], (int)hi[i][2], (int)hi[i][3]};
#pragma unroll
            for (int j = 0; j < FN; ++j)
              acc[i0 + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af, acc[i0 + i][j], 4, 0, 0,
                                                                                 ws[j], 0, kNeutral);
          }
        }
        store_a(kt + 1, ra[(s + 1) % AD]);
        __syncthreads();
      }
    }

    // lane: tile row i*16 + l16, columns wn0 + j*16 + 4g .. +3. The row scale belongs to the
    // SOURCE row: xscale[a_rows[r]] when the rows are gathered.
    float xs[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = m0 + i * 16 + l16;
      xs[i] = 0.f;
      if (m < out_rows) xs[i] = p.xscale[p.a_rows ? p.a_rows[r0 + m] : r0 + m];
    }
    if (p.act == ACT_SWIGLU) {
      // fragments (2jj, 2jj+1) of a lane: gate and up of the same four output columns
      const int NO = N / 2;
#pragma unroll
      for (int jj = 0; jj < FN / 2; ++jj) {
        const int ocol = wn0 / 2 + jj * 16 + 4 * g;
        if (ocol >= NO) continue;  // N % 32 == 0: a block pair is inside N or past it as a whole
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int m = m0 + i * 16 + l16;
          if (m >= out_rows) continue;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(silu(xs[i] * acc[i][2 * jj][e]) * (xs[i] * acc[i][2 * jj + 1][e]));
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
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int m = m0 + i * 16 + l16;
          if (m >= out_rows) continue;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(xs[i] * acc[i][j][e]);
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

// A block owns (group, column tile). G2 != G: the tile height goes by the group's own count, read
// on the device — up to G::BM rows take G's tile, more take the taller G2's (same waves and
// columns), so a busy group still crosses its weight panel once and a usual one pays no MFMAs for
// rows it does not have. The choice is made once per block, outside the K loop, which stays
// straight-line in both forms.
template <class G, class G2, bool SDW>
__global__ __launch_bounds__(G::T, G::OCC) void gemm_w4a8_grouped_kernel(const GW4Params p) {
  static_assert(G::T == G2::T && G::BN == G2::BN && G::BM <= G2::BM, "one grid, one block size");
  __shared__ u32x4 smem[2 * G2::A_UNITS];
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
  if constexpr (G::BM == G2::BM) {
    gw4_group<G, SDW>(p, smem, grp, tn, r0, count);
  } else {
    // (rows that are written: a compact output keeps at most compact_rows of them)
    if (min(count, p.c_ptrs != nullptr ? p.compact_rows : count) <= G::BM) gw4_group<G, SDW>(p, smem, grp, tn, r0, count);
    else gw4_group<G2, SDW>(p, smem, grp, tn, r0, count);
  }
}

using GW4C0 = GW4Cfg<32, 32, 4, 8, 4, 2>;    // short: small counts (few rows per expert)
using GW4C1 = GW4Cfg<128, 32, 4, 8, 2>;      // 128 rows x 128 columns, deep weight ring
using GW4C2 = GW4Cfg<128, 32, 8, 4, 2, 2>;   // 128 rows x 256 columns over 8 waves: one A tile feeds twice the columns
using GW4C3 = GW4Cfg<192, 32, 4, 8, 2>;      // 192 rows: a typical Mixtral expert in one pass over its weight panel
using GW4C4 = GW4Cfg<192, 32, 8, 4, 2, 2>;   // the same over 8 waves and 256 columns
using GW4T = GW4Cfg<256, 32, 4, 8, 2>;       // c5's tall form: 256 rows x 128 columns (64 KB of LDS)
// c5: c3 for groups of up to 192 rows, 256-row tiles for busier ones (a heavy Mixtral expert, 227
// rows, in one pass instead of two)
constexpr int kNumCfg = 6;
constexpr int kTileRows[kNumCfg] = {GW4C0::BM, GW4C1::BM, GW4C2::BM, GW4C3::BM, GW4C4::BM, GW4C3::BM};

template <class G, class G2 = G>
void launch_cfg(GW4Params p, bool sdw, hipStream_t s) {
  p.tiles_n = (p.N + G::BN - 1) / G::BN;
  const dim3 grid(p.groups * p.tiles_n), block(G::T);
  if (sdw) hipLaunchKernelGGL((gemm_w4a8_grouped_kernel<G, G2, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((gemm_w4a8_grouped_kernel<G, G2, false>), grid, block, 0, s, p);
}

}  // namespace

int gemm_w4a8_grouped_num_configs() { return kNumCfg; }

int gemm_w4a8_grouped_tile_rows(int cfg) { return kTileRows[cfg < 0 || cfg >= kNumCfg ? 0 : cfg]; }

int gemm_w4a8_grouped_pick(int rows_hint, int N, int K, int n_groups) {
  // Fitted to the cold-weight measurements of Mixtral's expert GEMMs (benchmarks/bench_grouped_w4a8.py,
  // profiles/mxfp4_experts/grouped_w4a8.txt), on the rule of gemm_w8_grouped_pick: the tile height
  // goes by the busiest group to expect, about 1.5 x the mean (rows_hint); 256 columns over 8 waves
  // when that still gives two rounds of blocks on the 256 CUs (gate/up), else 128 over 4 waves
  // (down: 256 blocks, long K) — there the form that sizes its tile by each group's own count, so
  // a layer with one heavy expert does not walk that expert's weight panel twice.
  (void)K;
  if (rows_hint <= 32) return 0;
  const bool wide = (long)n_groups * ((N + 255) / 256) >= 512;
  if (rows_hint <= 96) return wide ? 2 : 1;
  return wide ? 4 : 5;
}

void launch_gemm_w4a8_grouped(const GemmW4A8GroupedArgs& a, hipStream_t s) {
  if (a.n_groups <= 0 || a.R <= 0 || a.N <= 0 || a.K < 32) return;
  GW4Params p{};
  p.A = (const uint8_t*)a.Aq;
  p.lda = a.lda;
  p.xscale = a.xscale;
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
  const bool sdw = a.K % BK == 0 && a.scales_aligned4;
  switch (a.config) {
    case 0: launch_cfg<GW4C0>(p, sdw, s); break;
    case 1: launch_cfg<GW4C1>(p, sdw, s); break;
    case 2: launch_cfg<GW4C2>(p, sdw, s); break;
    case 3: launch_cfg<GW4C3>(p, sdw, s); break;
    case 4: launch_cfg<GW4C4>(p, sdw, s); break;
    default: launch_cfg<GW4C3, GW4T>(p, sdw, s); break;
  }
}
