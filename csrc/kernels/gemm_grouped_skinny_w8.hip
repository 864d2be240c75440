// Grouped skinny W8A16 GEMM (fp8 MoE experts of a decode step): the contract of
// launch_gemm_grouped_skinny with e4m3 weights and per-channel scales. Group g multiplies sorted
// rows [offsets[g], offsets[g+1]) of bf16 A (or, with a_rows, the token rows a_rows[r]) by its own
// weight w_ptrs[g] (e4m3 bytes, [N][K] contiguous), scales output channel n by s_ptrs[g][n] (fp32,
// any positive value, applied ONCE, after the fp32 accumulation) and writes the rows at the same
// rows of C, or compactly to rows 0..min(count, compact_rows)-1 of c_ptrs[g]. act: none or SwiGLU
// (rows of q AND scale gate/up-interleaved in blocks of 16). No bias, no residual. The arithmetic
// order is the epilogue of gemm_w8_grouped.hip: scale[n] * acc per fragment in fp32, then
// silu(gate) * up, then one rounding to bf16.
//
// The geometry, the K loop and the finish are gemm_skinny_impl.h's (the layout is explained there).
// Strip forms: a SwiGLU pair, 16 plain columns and 32 plain columns, each with W in {4, 8} waves and
// plain or nt weight loads: twelve instances (profiles/moe_skinny_w8/resources.txt).
//
// Two launches are bit-identical, and a group's row gives the same bits whether the group holds
// 1 row or 16.
#include "gemm_skinny_impl.h"

namespace {

using namespace dls_skinny;

struct GS8Params {
  const bf16* A;
  int lda;
  int a_total;  // rows of A (a_rows values are clamped to it)
  const int* a_rows;
  const int* offsets;
  const unsigned long long* w_ptrs;
  const unsigned long long* s_ptrs;
  const unsigned long long* c_ptrs;
  bf16* C;
  int ldc;
  int R, N, K;
  int compact_rows;
  int strips;
};

// One workgroup per (group, strip); the grid is (groups x strips), a function of the host shapes
// alone. A group with no rows returns before it reads w_ptrs[g] or s_ptrs[g] or forms a weight
// address, so a captured launch follows whatever routing the device holds at replay. A group of
// more than 16 rows takes further 16-row passes over the same weights (correct, not fast). A
// ragged last 32-column strip (N % 32 == 16) repeats weight row N - 1 in its second fragment and
// stores nothing for it. Pointers read from the device arrays (w_ptrs, s_ptrs, c_ptrs) go through
// the global address space: flat loads and stores would count against LDS waits too.
// FN: weight fragments per strip; SW: the two fragments are a gate/up pair (else FN x 16 plain
// columns); W: waves (K split); NT: streaming weight loads
template <int FN, bool SW, int W, bool NT>
__global__ __launch_bounds__(64 * W) void gemm_grouped_skinny_w8_kernel(const GS8Params p) {
  static_assert(!SW || FN == 2, "a SwiGLU strip is a gate/up fragment pair");
  __shared__ f32x4 red[(W - 1) * FN * 64];
  const auto [lane, wave, l16, g] = lanes();
  const int grp = blockIdx.x / p.strips, strip = blockIdx.x % p.strips;
  // offsets are clamped to [0, R], a_rows values (below) to [0, a_total - 1]
  const int r0 = min(max(p.offsets[grp], 0), p.R), r1 = min(max(p.offsets[grp + 1], 0), p.R);
  const int count = r1 - r0;
  if (count <= 0) return;  // before w_ptrs[grp] / s_ptrs[grp] are read or any weight address is formed
  const int K = p.K, N = p.N;

  global_bf16* Cg;
  int out_rows, crow0;
  if (p.c_ptrs != nullptr) {
    Cg = reinterpret_cast<global_bf16*>(p.c_ptrs[grp]);
    out_rows = min(count, p.compact_rows);
    crow0 = 0;
  } else {
    Cg = (global_bf16*)p.C;
    out_rows = count;
    crow0 = r0;
  }

  int s0, s1;
  run_of<W>(wave, K, s0, s1);
  const uint8_t* wp[FN];
  weight_rows(reinterpret_cast<const uint8_t*>(p.w_ptrs[grp]), (size_t)K, strip, l16, N, wp);
  global_f32* sp = reinterpret_cast<global_f32*>(p.s_ptrs[grp]);

  for (int m0 = 0; m0 < out_rows; m0 += 16) {
    if (m0 > 0) __syncthreads();  // the previous pass's sum has read `red`
    // token row of this lane's B column; columns past the count repeat the group's last row
    const int m = min(m0 + l16, count - 1);
    int src = p.a_rows ? p.a_rows[r0 + m] : r0 + m;
    src = min(max(src, 0), p.a_total - 1);
    const bf16* xp = p.A + (size_t)src * p.lda;

    f32x4 acc[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s0 < s1) run_k<FN, NT>(wp, xp, g, s0, s1, K, acc);  // wave-uniform

    // lane: token row m0 + l16, columns 4g..4g+3 of every fragment
    float sc[FN][4];
    if (wave > 0) {
      park(red, wave, lane, acc);
    } else {
      // value e of fragment j belongs to weight row strip * 16 FN + 16 j + 4g + e: its scale,
      // requested at clamped rows before the barrier
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[j][e] = sp[min(strip * 16 * FN + j * 16 + 4 * g + e, N - 1)];
    }
    __syncthreads();
    if (wave == 0) {
      sum_waves<FN, W>(red, lane, acc);
      const int row = m0 + l16;
      if (row < out_rows) {
        float v[FN][4];
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = sc[j][e] * acc[j][e];
        constexpr int NF = SW ? 1 : FN;  // output fragments of the strip
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          const int col = strip * 16 * NF + j * 16 + 4 * g;
          if (!SW && col >= N) continue;  // the second fragment of a ragged 32-column strip
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if constexpr (SW) o[e] = f2bf(silu(v[0][e]) * v[1][e]);
            else o[e] = f2bf(v[j][e]);
          }
          store4(Cg, (size_t)(crow0 + row) * p.ldc + col, p.ldc, o, 4);
        }
      }
    }
  }
}

template <int FN, bool SW>
void launch(const GS8Params& p, int blocks, int waves, bool nt, hipStream_t s) {
  by_waves<8, 4>(waves, [&](auto w) {
    by_bool(nt, [&](auto t) {
      hipLaunchKernelGGL((gemm_grouped_skinny_w8_kernel<FN, SW, w(), t()>), dim3(blocks), dim3(64 * w()), 0, s, p);
    });
  });
}

}  // namespace

bool gemm_grouped_skinny_w8_takes(int N, int K, int act) {
  if (act != 0 && act != kActSwiglu) return false;
  if (N <= 0 || K <= 0 || K % 32 != 0) return false;
  return act == kActSwiglu ? N % 32 == 0 : N % 16 == 0;
}

// The instance rule, read off the kernel table of profiles/moe_skinny_w8/kernels.txt (Mixtral's
// shapes, M = 1, 4, 8, 16; README, "fp8-expert skinny grouped GEMM") and mirrored by
// ops.grouped_skinny_w8_waves / _strip / _nt:
//  - plain loads: nt lost in every one of the 48 pairs, by 4 to 22 % (the dense fp8 kernel's finding);
//  - SwiGLU (K 4096, 32 slices): four waves, 43 against 56 us at M = 1 and 17 to 19 % ahead above;
//  - plain strips: 32 columns — ahead of 16 at every M but W 4 at M = 1 (30.4 against 29.7 us) —
//    with eight waves from 64 slices on (K 14336: 22.1 against 30.4 us at M = 1, the rows the
//    executor sends here; at M >= 4 four waves lead by 4 to 5 %). Below 64 slices no plain shape
//    was measured; four waves there is the dense fp8 kernel's rule, not a measurement.
int gemm_grouped_skinny_w8_waves(int N, int K, int act) {
  (void)N;
  if (act == kActSwiglu) return 4;
  return (K + BK - 1) / BK >= 64 ? 8 : 4;
}

int gemm_grouped_skinny_w8_strip(int N, int K, int act) {
  (void)N;
  (void)K;
  return act == kActSwiglu ? 16 : 32;
}

bool gemm_grouped_skinny_w8_nt(int N, int K, int act) {
  (void)N;
  (void)K;
  (void)act;
  return false;
}

bool launch_gemm_grouped_skinny_w8(const GemmGroupedSkinnyW8Args& a, hipStream_t s) {
  if (a.n_groups <= 0 || a.R <= 0 || a.a_total <= 0 || !gemm_grouped_skinny_w8_takes(a.N, a.K, a.act)) return false;
  if (a.w_ptrs == nullptr || a.s_ptrs == nullptr) return false;
  if (a.waves != 0 && a.waves != 4 && a.waves != 8) return false;
  if (a.strip != 0 && a.strip != 16 && a.strip != 32) return false;
  if (a.act == kActSwiglu && a.strip == 32) return false;  // a SwiGLU strip is the 16-output pair
  GS8Params p{};
  p.A = (const bf16*)a.A;
  p.lda = a.lda;
  p.a_total = a.a_total;
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
  p.compact_rows = a.compact_rows;
  const int waves = a.waves ? a.waves : gemm_grouped_skinny_w8_waves(a.N, a.K, a.act);
  const int strip = a.strip ? a.strip : gemm_grouped_skinny_w8_strip(a.N, a.K, a.act);
  const bool nt = a.nt < 0 ? gemm_grouped_skinny_w8_nt(a.N, a.K, a.act) : a.nt != 0;
  if (a.act == kActSwiglu) {
    p.strips = a.N / 32;
    launch<2, true>(p, a.n_groups * p.strips, waves, nt, s);
  } else if (strip == 32) {
    p.strips = (a.N + 31) / 32;
    launch<2, false>(p, a.n_groups * p.strips, waves, nt, s);
  } else {
    p.strips = a.N / 16;
    launch<1, false>(p, a.n_groups * p.strips, waves, nt, s);
  }
  return true;
}
