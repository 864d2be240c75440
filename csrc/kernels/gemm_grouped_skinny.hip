// Grouped skinny GEMM (MoE experts of a decode step): the contract of launch_gemm_glds_grouped
// for bf16 without bias or residual, act in {none, SwiGLU}, built for groups of AT MOST 16 rows.
// Group g multiplies sorted rows [offsets[g], offsets[g+1]) of A (or, with a_rows, the token rows
// a_rows[r]) by its own weight w_ptrs[g] ([N][K]) and writes them at the same rows of C, or
// compactly to rows 0..min(count, compact_rows)-1 of c_ptrs[g].
//
// A decode step has M = B*T <= 16 token rows, every expert gets at most M of them and most
// experts get none, so the launch is a weight stream: each routed weight byte is needed once, by
// one wave, and the arithmetic is free. The loop is the "GEMV / M <= 16 decode weights" form:
// weights go global -> VGPR with 16-byte streaming (nt) loads through a two-slot register ring in
// a straight-line unrolled body; no LDS in the K loop and no barrier. What keeps bytes in flight
// is OCCUPANCY, five to eight waves per SIMD, not the ring: in the generated code the first wait
// of every loop trip is vmcnt(0) (see the loop), so inside one wave a trip's loads do not overlap
// the next trip's. A counted, late wait across trips is what the loop is written for and what
// the compiler does not emit.
//
// Work split. A workgroup owns one (group, column strip): 16 output columns — for SwiGLU one
// 16-gate + 16-up block pair of the interleaved weight, which is 16 outputs too. Its four waves
// split K in contiguous runs of 64-wide slices, each holds a 16 x 16 fp32 fragment (two for
// SwiGLU) of the strip, and the finish is one LDS exchange: waves 1..3 park their fragments, one
// barrier, wave 0 adds them to its own IN ASCENDING WAVE ORDER, applies SiLU(gate) * up or the
// identity in fp32, rounds once to bf16 and stores. No atomics and no split-K across workgroups:
// the same launch twice is bit-identical. The grid is (groups x strips), a function of the host
// shapes alone; a group with no rows returns before it requests a weight byte, so a captured
// launch follows whatever routing the device holds at replay. A group of more than 16 rows takes
// further 16-row passes over the same weights (correct, not fast).
//
// Operand layout. Operands are swapped as in gemm_w8_grouped.hip and attn_decode.hip: the weight
// rows are the MFMA's A operand (lane l16 = weight row), the <= 16 token rows its B operand
// (lane l16 = token), so a lane's four accumulator values are four CONSECUTIVE output columns of
// one token row — one 8-byte store — and a gate/up pair is two fragments of the same lane. The
// MFMA's own k map gives lane group g = lane >> 4 the 8 values k = 8g..8g+7 of a 32-wide step:
// 16 bytes per lane, 64 contiguous bytes per weight row, half a cache line. A sum over k does
// not care which k a lane holds as long as both operands agree, so a slice is 64 wide and lane
// group g takes k = 16g..16g+15 of it — two adjacent 16-byte loads, 32 contiguous bytes — feeding
// MFMA step h with its k = 16g + 8h ..+7. A wave's load pair then covers 16 whole 128-byte lines
// of the weight, each requested exactly once. The token operand uses the same map and is read
// straight from global memory as well: the rows are a few KB that every strip of the launch
// re-reads, so they sit in L2, and with fewer than 16 rows the lanes of the missing rows repeat
// the group's last row (same address, no extra traffic). A column of the B operand only reaches
// its own token's outputs, so whatever a clamped lane reads never reaches a stored element.
#include "common.h"
#include "kernels.h"

namespace {

// as in gemm_w8_grouped.hip: addresses that come from a device array need the global address
// space spelled out, or the loads are FLAT and count against LDS waits too
typedef const __attribute__((address_space(1))) u32x4 global_u32x4;

constexpr int BK = 64;     // K slice: one 128-byte line per weight row
constexpr int WAVES = 4;   // K split of a strip
// Slices in a wave's register ring. Two: 76 (SwiGLU) / 54 VGPRs, five to eight waves per SIMD, and
// it is the waves of several workgroups per CU, each with 8 or 12 loads in flight, that keep the
// bytes coming while one of them is in its prologue or its finish. Measured on an MI355X at
// Mixtral's shapes against rings of 4, 6 and 8 slices (three, two and one wave per SIMD): 2 and 4
// tie on gate/up, 6 and 8 are 8-25 % slower; on down 2 is the fastest at M = 1 (47 against
// 56 us) and ties 4 above.
constexpr int PF = 2;

struct GSParams {
  const bf16* A;
  int lda;
  int a_total;  // rows of A (a_rows values are clamped to it)
  const int* a_rows;
  const int* offsets;
  const unsigned long long* w_ptrs;
  const unsigned long long* c_ptrs;
  bf16* C;
  int ldc;
  int R, N, K;
  int compact_rows;
  int strips;
};

// FN: weight fragments per strip (1 plain, 2 SwiGLU: gate block + up block)
template <int FN>
__global__ __launch_bounds__(64 * WAVES) void gemm_grouped_skinny_kernel(const GSParams p) {
  __shared__ f32x4 red[(WAVES - 1) * FN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // in an SGPR: the K loop's branches are scalar
  const int l16 = lane & 15, g = lane >> 4;
  const int grp = blockIdx.x / p.strips, strip = blockIdx.x % p.strips;
  const int r0 = min(max(p.offsets[grp], 0), p.R), r1 = min(max(p.offsets[grp + 1], 0), p.R);
  const int count = r1 - r0;
  if (count <= 0) return;  // before any weight address is formed
  const int K = p.K;

  bf16* Cg;
  int out_rows, crow0;
  if (p.c_ptrs != nullptr) {
    Cg = reinterpret_cast<bf16*>(p.c_ptrs[grp]);
    out_rows = min(count, p.compact_rows);
    crow0 = 0;
  } else {
    Cg = p.C;
    out_rows = count;
    crow0 = r0;
  }

  // this wave's run of slices; K % 32 == 0, so the last slice is whole or its lane groups 2, 3
  // are past K
  const int nk = (K + BK - 1) / BK, per = (nk + WAVES - 1) / WAVES;
  const int s0 = wave * per, s1 = min(nk, s0 + per);

  // lane (l16, g): bytes [32g, 32g + 32) of the line of weight row l16 of every fragment. Loads
  // are unconditional at clamped addresses (slices past the run repeat its last slice, which is
  // in flight or cached; k past K repeats the row's last 32 bytes) and what must not count is
  // zeroed where it is consumed — a select behind the load would make the wave wait at once.
  const unsigned long long W = p.w_ptrs[grp];
  unsigned long long wp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = W + (unsigned long long)(strip * 16 * FN + j * 16 + l16) * K * 2;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

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

    if (s0 < s1) {  // wave-uniform
      u32x4 wr[PF][FN][2], xr[PF][2];
      auto load = [&](int kt, u32x4(&w)[FN][2], u32x4(&x)[2]) {
        const int ko = min(min(kt, s1 - 1) * BK + 16 * g, K - 16);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          global_u32x4* q = reinterpret_cast<global_u32x4*>(wp[j] + (unsigned long long)ko * 2);
          w[j][0] = __builtin_nontemporal_load(q);
          w[j][1] = __builtin_nontemporal_load(q + 1);
        }
        const u32x4* q = reinterpret_cast<const u32x4*>(xp + ko);
        x[0] = q[0];
        x[1] = q[1];
      };
      auto mma = [&](const u32x4(&w)[FN][2], const u32x4(&x)[2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&x[h]);
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[j] = mfma16x16x32(*reinterpret_cast<const bf16x8*>(&w[j][h]), xf, acc[j]);
        }
      };
      // Main loop: PF whole slices inside the run per trip (the run's last slice, the only one
      // that can reach past K, is always left to the tail). Slice kt's MFMAs read ring slot
      // kt % PF, then the slot is refilled with slice kt + PF. The scheduling barriers keep that
      // order in the code: with it the compiler's wait before a slice's MFMAs inside a trip is
      // the counted vmcnt that leaves the PF - 1 younger slices in flight, and the ring stays in
      // place (left alone, the scheduler sank a trip's loads behind all its MFMAs and renamed the
      // ring into 232 VGPRs). The first wait of every trip is still vmcnt(0) in the generated code
      // (the loop header's merge): one more reason the bytes in flight come from many waves.
      int kt0 = s0;
#pragma unroll
      for (int s = 0; s < PF; ++s) {
        load(s0 + s, wr[s], xr[s]);
        __builtin_amdgcn_sched_barrier(0);  // slot by slot: slice s0's loads are the oldest
      }
      for (; kt0 + PF < s1; kt0 += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
          __builtin_amdgcn_sched_barrier(0);
          mma(wr[s], xr[s]);
          __builtin_amdgcn_sched_barrier(0);
          load(kt0 + s + PF, wr[s], xr[s]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // the last (up to) PF slices: nothing left to request; what is past the run or past K is zeroed
#pragma unroll
      for (int s = 0; s < PF; ++s) {
        const int kt = kt0 + s;
        const bool in = kt < s1 && kt * BK + 16 * g < K;
        u32x4 w[FN][2], x[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          x[h] = in ? xr[s][h] : zero4;
#pragma unroll
          for (int j = 0; j < FN; ++j) w[j][h] = in ? wr[s][j][h] : zero4;
        }
        mma(w, x);
      }
    }

    // lane: token row m0 + l16, columns 4g..4g+3 of the strip
    if (wave > 0) {
#pragma unroll
      for (int j = 0; j < FN; ++j) red[((wave - 1) * FN + j) * 64 + lane] = acc[j];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < WAVES - 1; ++w)  // ascending wave order
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const f32x4 t = red[(w * FN + j) * 64 + lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] += t[e];
        }
      const int row = m0 + l16;
      if (row < out_rows) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (FN == 2) o[e] = f2bf(silu(acc[0][e]) * acc[1][e]);
          else o[e] = f2bf(acc[0][e]);
        }
        const size_t idx = (size_t)(crow0 + row) * p.ldc + strip * 16 + 4 * g;
        if ((p.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(Cg) & 7) == 0)) {
          *reinterpret_cast<bf16x4*>(Cg + idx) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) Cg[idx + e] = o[e];
        }
      }
    }
  }
}

}  // namespace

bool gemm_grouped_skinny_takes(int N, int K, int act) {
  if (act != 0 && act != kActSwiglu) return false;
  if (N <= 0 || K <= 0 || K % 32 != 0) return false;
  return act == kActSwiglu ? N % 32 == 0 : N % 16 == 0;
}

void launch_gemm_grouped_skinny(const GemmGroupedSkinnyArgs& a, hipStream_t s) {
  if (a.n_groups <= 0 || a.R <= 0 || a.a_total <= 0 || !gemm_grouped_skinny_takes(a.N, a.K, a.act)) return;
  GSParams p{};
  p.A = (const bf16*)a.A;
  p.lda = a.lda;
  p.a_total = a.a_total;
  p.a_rows = a.a_rows;
  p.offsets = a.offsets;
  p.w_ptrs = a.w_ptrs;
  p.c_ptrs = a.c_ptrs;
  p.C = (bf16*)a.C;
  p.ldc = a.ldc;
  p.R = a.R;
  p.N = a.N;
  p.K = a.K;
  p.compact_rows = a.compact_rows;
  if (a.act == kActSwiglu) {
    p.strips = a.N / 32;
    hipLaunchKernelGGL((gemm_grouped_skinny_kernel<2>), dim3(a.n_groups * p.strips), dim3(64 * WAVES), 0, s, p);
  } else {
    p.strips = a.N / 16;
    hipLaunchKernelGGL((gemm_grouped_skinny_kernel<1>), dim3(a.n_groups * p.strips), dim3(64 * WAVES), 0, s, p);
  }
}
