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
// It is the skeleton of gemm_grouped_skinny.hip laid out again for 1-byte weights, as
// gemm_skinny_w8.hip did for the dense kernel: the launch is a weight stream, every routed weight
// byte is needed once, by one wave.
//
// Grid. A workgroup owns one (group, column strip); the grid is (groups x strips), a function of
// the host shapes alone. A group with no rows returns before it reads w_ptrs[g] or s_ptrs[g] or
// forms a weight address, so a captured launch follows whatever routing the device holds at
// replay. A group of more than 16 rows takes further 16-row passes (correct, not fast).
//
// Strip forms (template parameters FN, SW): a SwiGLU pair (16 gate + 16 up rows of the interleaved
// weight, two fragments sharing one token fragment, 16 outputs), a plain strip of 16 columns, and
// a plain strip of 32 columns (two fragments sharing one token fragment: per lane two weight
// requests for every token request, where the 16-column form has one for two). A ragged last
// 32-column strip (N % 32 == 16) repeats weight row N - 1 in its second fragment and stores
// nothing for it. W in {4, 8} waves split K: six instances, each with plain or nt weight loads.
//
// K loop. Slices are 128 wide: one 128-byte line per weight row. Weight rows are the MFMA's A
// operand (lane l16 = weight row), token rows its B operand (lane l16 = token), so a lane's four
// accumulator values are four CONSECUTIVE output columns of one token row. Lane (l16, g) loads
// bytes [32g, 32g + 32) of weight row l16 as two adjacent 16-byte global -> VGPR loads — a wave's
// load pair covers 16 whole lines, each requested once — converts them in registers with
// cvt_e4m3x8 (exact for all finite codes) and feeds four v_mfma_f32_16x16x32_bf16 steps: step h
// uses k = 32g + 8h..+7 of the slice on both operands. The token operand (four 16-byte loads per
// slice) is read from global memory / L2 with the same k map; lanes of missing rows repeat the
// group's last row (same address; a B column only reaches its own token's outputs, so what a
// clamped lane reads is never stored). The W waves take contiguous runs of slices through a
// two-slot register ring in a straight-line body pinned with sched_barrier(0). Loads are
// unconditional at clamped addresses (min(ko, K - 32); slices past the run repeat its last slice)
// and values are zeroed where they are consumed. No LDS and no barrier inside the K loop.
//
// What the compiler emits for the waits (-O3, gfx950, read from the ISA of all twelve
// instantiations; profiles/moe_skinny_w8/resources.txt): the ring stays in place, no instance uses
// scratch, every load and store is global_* (none flat). A slot holds 2 FN weight + 4 token
// loads. BOTH waits of a trip are counted: in front of slot 0's MFMAs, the first wait of the
// trip, the wave waits in steps down to vmcnt(4 + 2 FN) — vmcnt(14), (12), (8) with two
// fragments, vmcnt(10), (6) with one — which leaves slot 1's whole refill of the previous trip in
// flight, and the same sequence stands in front of slot 1's MFMAs, leaving slot 0's refill in
// flight. No vmcnt(0) inside the loop (the bf16 grouped kernel's first wait per trip is one).
// The only vmcnt(0) before the loop is the one for the a_rows / offsets reads that form the
// token address, ahead of the prologue's loads; the tail waits vmcnt(4 + 2 FN) once more, then
// drains.
//
// Pointers read from the device arrays (w_ptrs, s_ptrs, c_ptrs) go through the global address
// space: flat loads and stores would count against LDS waits too.
//
// Finish. Waves 1.. park their fp32 fragments in LDS; wave 0 requests its 4 scales per fragment
// before it waits at the one barrier, adds the fragments IN ASCENDING WAVE ORDER, applies scale,
// then SwiGLU or the identity, rounds once and stores 8 bytes per fragment where alignment allows,
// else element-wise. No atomics, no split-K across workgroups, no workspace: two launches are
// bit-identical, and a group's row gives the same bits whether the group holds 1 row or 16.
#include "common.h"
#include "kernels.h"

namespace {

typedef const __attribute__((address_space(1))) u32x4 global_u32x4;
typedef const __attribute__((address_space(1))) float global_f32;
typedef __attribute__((address_space(1))) bf16 global_bf16;
typedef __attribute__((address_space(1))) bf16x4 global_bf16x4;

constexpr int BK = 128;  // K slice: one 128-byte line per weight row
constexpr int LK = 32;   // k of a slice per lane group: 32 weight bytes, 64 bytes of x
constexpr int PF = 2;    // slices in a wave's register ring (see gemm_grouped_skinny.hip)

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

// One wave's run of slices [s0, s1) of one 16-row pass: acc[j] += W_j x^T over the run (always
// inlined: the ring and the fragments are registers of the kernel).
template <int FN, bool NT>
__device__ __forceinline__ void run_k(const unsigned long long (&wp)[FN], const bf16* xp, int g, int s0,
                                                int s1, int K, f32x4 (&acc)[FN]) {
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 wr[PF][FN][2], xr[PF][4];
  auto load = [&](int kt, u32x4(&w)[FN][2], u32x4(&x)[4]) {
    const int ko = min(min(kt, s1 - 1) * BK + LK * g, K - LK);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      global_u32x4* q = reinterpret_cast<global_u32x4*>(wp[j] + (unsigned long long)ko);
      if constexpr (NT) {
        w[j][0] = __builtin_nontemporal_load(q);
        w[j][1] = __builtin_nontemporal_load(q + 1);
      } else {
        w[j][0] = q[0];
        w[j][1] = q[1];
      }
    }
    const u32x4* q = reinterpret_cast<const u32x4*>(xp + ko);
#pragma unroll
    for (int h = 0; h < 4; ++h) x[h] = q[h];
  };
  auto mma = [&](const u32x4(&w)[FN][2], const u32x4(&x)[4]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&x[h]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[j] = mfma16x16x32(cvt_e4m3x8(w[j][h >> 1][2 * (h & 1)], w[j][h >> 1][2 * (h & 1) + 1]), xf, acc[j]);
    }
  };
  // Main loop: PF whole slices inside the run per trip; the run's last slice, the only one that
  // can reach past K, is always left to the tail. A slot's loads are issued right after its MFMAs,
  // so the wait in front of the other slot's MFMAs leaves them in flight.
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
  // (an e4m3 zero byte converts to +0, and x is zeroed too: a NaN past K must not meet it)
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    const int kt = kt0 + s;
    const bool in = kt < s1 && kt * BK + LK * g < K;
    u32x4 w[FN][2], x[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) x[h] = in ? xr[s][h] : zero4;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < FN; ++j) w[j][h] = in ? wr[s][j][h] : zero4;
    mma(w, x);
  }
}

// FN: weight fragments per strip; SW: the two fragments are a gate/up pair (else FN x 16 plain
// columns); W: waves (K split); NT: streaming weight loads
template <int FN, bool SW, int W, bool NT>
__global__ __launch_bounds__(64 * W) void gemm_grouped_skinny_w8_kernel(const GS8Params p) {
  static_assert(!SW || FN == 2, "a SwiGLU strip is a gate/up fragment pair");
  __shared__ f32x4 red[(W - 1) * FN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // in an SGPR: the K loop's branches are scalar
  const int l16 = lane & 15, g = lane >> 4;
  const int grp = blockIdx.x / p.strips, strip = blockIdx.x % p.strips;
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

  // this wave's run of slices; K % 32 == 0, so a lane group of the last slice is whole or past K
  const int nk = (K + BK - 1) / BK, per = (nk + W - 1) / W;
  const int s0 = wave * per, s1 = min(nk, s0 + per);

  // lane (l16, g): bytes [32g, 32g + 32) of the line of weight row l16 of every fragment; rows
  // past N (the second fragment of a ragged 32-column strip) repeat row N - 1
  const unsigned long long Wb = p.w_ptrs[grp];
  unsigned long long wp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = Wb + (unsigned long long)min(strip * 16 * FN + j * 16 + l16, N - 1) * K;
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
#pragma unroll
      for (int j = 0; j < FN; ++j) red[((wave - 1) * FN + j) * 64 + lane] = acc[j];
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
#pragma unroll 3
      for (int w = 0; w < W - 1; ++w)  // ascending wave order
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const f32x4 t = red[(w * FN + j) * 64 + lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] += t[e];
        }
      const int row = m0 + l16;
      if (row < out_rows) {
        float v[FN][4];
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = sc[j][e] * acc[j][e];
        constexpr int NF = SW ? 1 : FN;  // output fragments of the strip
        const bool wide = (p.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(Cg) & 7) == 0);
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
          const size_t idx = (size_t)(crow0 + row) * p.ldc + col;
          if (wide) {
            *reinterpret_cast<global_bf16x4*>(Cg + idx) = o;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) Cg[idx + e] = o[e];
          }
        }
      }
    }
  }
}

template <int FN, bool SW, int W>
void launch_nt(const GS8Params& p, int blocks, bool nt, hipStream_t s) {
  if (nt) hipLaunchKernelGGL((gemm_grouped_skinny_w8_kernel<FN, SW, W, true>), dim3(blocks), dim3(64 * W), 0, s, p);
  else hipLaunchKernelGGL((gemm_grouped_skinny_w8_kernel<FN, SW, W, false>), dim3(blocks), dim3(64 * W), 0, s, p);
}

template <int FN, bool SW>
void launch_w(const GS8Params& p, int blocks, int waves, bool nt, hipStream_t s) {
  if (waves == 8) launch_nt<FN, SW, 8>(p, blocks, nt, s);
  else launch_nt<FN, SW, 4>(p, blocks, nt, s);
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
    launch_w<2, true>(p, a.n_groups * p.strips, waves, nt, s);
  } else if (strip == 32) {
    p.strips = (a.N + 31) / 32;
    launch_w<2, false>(p, a.n_groups * p.strips, waves, nt, s);
  } else {
    p.strips = a.N / 16;
    launch_w<1, false>(p, a.n_groups * p.strips, waves, nt, s);
  }
  return true;
}
