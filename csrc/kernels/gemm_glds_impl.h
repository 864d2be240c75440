// gemm_glds_impl.h: the LDS-DMA GEMM's device code and per-config launcher, included by the
// per-config translation units gemm_glds_cfg*.hip (compiled in parallel) — see gemm_glds.hip.
#pragma once
// Multistage bf16 GEMM with LDS-DMA staging (global_load_lds_dwordx4), optional split-K.
//
//   C = act(alpha * A @ W^T + bias) + R      A [M][K], W [N][K] (K contiguous), K % 64 == 0
//
// Why this structure (cdna_hip_programming.md §5 "Pipelining across barriers", T1, T2):
//  * GPT-2 / Llama serving GEMMs have M = 512 rows: a grid barely covers the 256 CUs, so
//    each CU runs ~1 block and a K-loop that keeps ONE tile in flight is latency-bound —
//    especially when the weights stream cold from HBM (measured 1.6-2x slower inside the
//    DAG than in a hot-cache loop). Here STAGES-1 K-tiles are in flight per block.
//  * LDS-DMA needs no staging VGPRs and no ds_write pass; the image is lane-linear (1 KiB
//    per wave instruction = 8 rows x 128 B), so the XOR swizzle (chunk ^ (row & 7)) is
//    applied to the per-lane SOURCE address and again on the ds_read (rule 21).
//  * ONE raw s_barrier per K-tile: wait(tile kt) -> barrier -> issue(tile kt+STAGES-1 into
//    the buffer everyone finished reading before this barrier) -> MFMAs on tile kt. The
//    wait is a counted vmcnt (never 0 in steady state); __syncthreads() is avoided because
//    its fence drains every outstanding DMA.
//  * Split-K (host-chosen) multiplies the block count for skinny N; partial fp32 tiles go
//    to a workspace slab and a vectorised reduce kernel applies the fused epilogue.
//  * XCD-aware tile order (T1): the blocks of one weight panel share an XCD's L2.
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "kernels.h"
#include "gemm_glds_cfgs.h"

// In-kernel phase stamps for diagnostic builds (benchmarks/gemm_stamps.hip defines it before
// including this file); empty in the library. glds_tile stamps 0 tile start, 1 after the main
// loop, 7 after the K-group sum (one-pass finish: after every K group's fragments are in LDS),
// 2 after the output image is in LDS (never on the one-pass finish: it has no image), 3 after
// the stores (4-6 belong to gemm_fused.hip).
#ifndef DLS_STAMP
#define DLS_STAMP(k)
#endif

namespace {

__device__ __forceinline__ int kslice_count(int K, int kslice) { return K / kslice; }

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// wait until at most `ahead` tiles (PW DMA instructions each) are still in flight; the
// immediate must be a compile-time constant, so unroll over the possible values
template <int PW, int A>
__device__ __forceinline__ void wait_tiles(int ahead) {
  if constexpr (A == 0) {
    wait_vm<0>();
  } else {
    if (ahead >= A) wait_vm<PW * A>();
    else wait_tiles<PW, A - 1>(ahead);
  }
}
__device__ __forceinline__ void raw_barrier() { asm volatile("s_barrier" ::: "memory"); }
// Workgroup barrier of the epilogue's LDS hand-offs: the wave's own LDS traffic is complete
// (lgkmcnt(0)) before it arrives. WAIT_LDS_ONLY leaves its global loads in flight — the
// __syncthreads() fence puts a vmcnt(0) in front of the barrier, which would end the batched
// epilogue operand requests (Cfg::EPI_BATCH) at the first barrier after them.
// A value requested earlier is consumed from HERE on: the (empty) statement is its first use,
// so the compiler's vmcnt wait for the load lands at this point and no arithmetic on the value
// can be moved up to the request (InstCombine folds an operation on a phi of {constant, load}
// into the load's block — a wait right behind the request).
template <class T>
__device__ __forceinline__ void consume_from_here(T& x) {
  asm volatile("" : "+v"(x));
}
// One output value of the one-pass finishes (glds_tile, gemm_private_wide_kernel) before RoPE and
// rounding: x the K sum, b the bias, and with a folded norm (LNM) the row's rstd / mean and the
// column's colsum(W') — W.LN(x) = rstd * (W' x - mu * colsum(W')) + (bias + W b), W' = W * ln_w
// (host-derived) — else alpha.
template <int ACT, bool LNM>
__device__ __forceinline__ float finish_value(float x, float alpha, float rs, float mu, float cs, float b) {
  if constexpr (LNM) return act_c<ACT>(rs * (x - mu * cs) + b);
  else return act_c<ACT>(alpha * x + b);
}
template <bool WAIT_LDS_ONLY>
__device__ __forceinline__ void epi_barrier() {
  if constexpr (WAIT_LDS_ONLY) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else __syncthreads();
}

// BXS = extra weight (B) stages: 0 -> A and W tiles share STAGES buffers and travel
// together; >= 1 -> A keeps STAGES buffers (it is L2-resident: short latency) while the COLD
// weight stream gets STAGES + BXS, i.e. BXS more tiles of HBM latency covered inside the same
// 160 KiB of LDS (e.g. 256x256: 2 x 32 KiB A + 3 x 32 KiB W).
// KG_ = K groups: KG wave groups of WM x WN waves share each output tile; a stage holds KG
// consecutive 64-deep K-tiles and group g multiplies tile g of every stage (intra-block
// split-K: KG x the waves — and DMA issuers — per CU on a skinny grid, no reduce kernel; the
// groups' accumulators meet in LDS after the K loop: the small wave tiles sum and finish them
// there in one pass by every thread (ONE_PASS below), the others sum them into group 0, which
// runs the staged epilogue).
// RING_ = 1: the 256x256 half-tile ring main loop (mainloop_ring) instead of whole-K-tile stages
// OCC_: waves per SIMD the kernel must allow (__launch_bounds__' second argument): 2 for the
// 4-wave tiles meant to run two workgroups per CU (at most 256 VGPRs + AGPRs per wave)
template <int BM_, int BN_, int WM_, int WN_, int STAGES_, int PRIO_ = 0, int BXS_ = 0, int KG_ = 1, int RING_ = 0,
          int OCC_ = 1>
struct Cfg {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, STAGES = STAGES_, PRIO = PRIO_, BXS = BXS_;
  static constexpr int KG = KG_, RING = RING_, OCC = OCC_;
  static constexpr int BK = 64, CH = 8;
  static constexpr int NW = WM * WN, T = 64 * NW * KG;
  static constexpr int WTM = BM / WM, WTN = BN / WN, FM = WTM / 16, FN = WTN / 16;
  // fragments of one 32-deep K half at a time (instead of both halves before the first MFMA)
  // for wave tiles with many fragments (32 x 224)
  static constexpr bool HALF_FRAGS = FM + FN > 12;
  // DMA instructions (8 rows x 128 B each) per wave: when the rows do not split evenly over
  // the waves, the last waves repeat the stage's last instruction (same bytes to the same LDS
  // slot), so every wave issues the same count and the counted vmcnt waits stay uniform
  static constexpr int ROWS = BM + BN, INSTR = ROWS / 8, PW = (INSTR + NW - 1) / NW;
  static constexpr int SUB = ROWS * CH;     // one 64-deep K-tile image (bf16x8 units)
  static constexpr int STAGE = SUB * KG;    // bf16x8 units
  // split staging (BXS > 0): separate A / W rings
  static constexpr int SA = STAGES, SB = STAGES + BXS;
  static constexpr int PWA = (BM / 8 + NW - 1) / NW, PWB = (BN / 8 + NW - 1) / NW;
  static constexpr bool EVEN = INSTR % NW == 0, EVEN_A = (BM / 8) % NW == 0, EVEN_B = (BN / 8) % NW == 0;
  static constexpr int A_STAGE = BM * CH, B_STAGE = BN * CH;
  static constexpr int LDS_UNITS = BXS ? SA * A_STAGE + SB * B_STAGE : STAGES * STAGE;
  static_assert(BM % 8 == 0 && BN % 8 == 0, "DMA pieces are 8 rows");
  static_assert(FM >= 1 && FN >= 1, "wave tile too small");
  static_assert(PW * (STAGES - 2) <= 63, "vmcnt range");
  static_assert(!BXS || (SA - 2) * PWA + (SA - 1) * PWB <= 63, "vmcnt range (split rings)");
  static_assert(STAGES >= 2 && STAGES <= 8, "stages");
  static_assert(LDS_UNITS * 16 <= 163840, "LDS budget");
  static_assert(KG == 1 || (BXS == 0 && PRIO == 0), "K groups use the joint ring");
  // K-group sum into group 0 (split-K slices, SwiGLU, tiles without ONE_PASS): one LDS region of
  // NW * FM * FN KiB per K group past the first (all written before ONE barrier)
  static_assert(KG == 1 || (KG - 1) * NW * 64 * FM * FN * 16 <= LDS_UNITS * 16, "K-group reduction must fit the LDS");
  // Batched epilogue operand requests (glds_tile): the small wave tiles of the skinny M = 512
  // GEMMs, whose body is a few us and whose epilogue operands (row statistics, bias, colsum,
  // residual) otherwise arrive one dependent round trip after another behind barriers. At most
  // 4 accumulator fragments per lane: the requests' 20-odd destination registers are free there.
  // The large tiles (128 accumulator registers and more next to their fragment registers) keep
  // the in-place loads — their epilogue is a small share of a long body.
  static constexpr bool EPI_BATCH = FM * FN <= 4;
  // One-pass finish of a K-grouped tile (glds_tile): EVERY K group writes its fp32 fragments to
  // an LDS region of its own, one barrier, and every thread of the block sums, finishes and
  // stores one 16-byte row segment — instead of K group 0 summing the others' fragments,
  // writing a bf16 tile image to LDS and the block reading that back (two trips through LDS, the
  // finishing arithmetic on 1 / KG of the waves). Configs 16, 17, 20, 27 and 45; a config that
  // loses with it is gated out here.
  static constexpr bool ONE_PASS = KG > 1 && EPI_BATCH;
  static_assert(!ONE_PASS || KG * NW * 64 * FM * FN * 16 <= LDS_UNITS * 16, "one region per K group must fit the LDS");
  static_assert(!RING || (BM == 256 && BN == 256 && WM == 2 && WN == 4 && STAGES == 2 && KG == 1 && BXS == 0),
                "the ring main loop is written for 256x256 tiles, 8 waves as 2 x 4, 8 x 16 KiB slots");
};

// split rings with a W ring D = BXS tiles deeper than the A ring: wait until at most
// a*PWA + b*PWB DMA instructions are outstanding, a in [0, AM], b in [0, BM] (any pair)
template <int PWA, int PWB, int AM, int BM>
__device__ __forceinline__ void wait_ab_any(int a, int b) {
  if constexpr (AM > 0) {
    if (a < AM) {
      wait_ab_any<PWA, PWB, AM - 1, BM>(a, b);
      return;
    }
  }
  if constexpr (BM > 0) {
    if (b < BM) {
      wait_ab_any<PWA, PWB, AM, BM - 1>(a, b);
      return;
    }
  }
  wait_vm<AM * PWA + BM * PWB>();
}
// split rings: wait until at most a*PWA + b*PWB DMA instructions are outstanding, with
// a in [0, AMAX] and b in {a, a + 1} (see the issue order in glds_tile)
template <int PWA, int PWB, int A>
__device__ __forceinline__ void wait_ab(int a, int b) {
  if constexpr (A == 0) {
    if (b >= 1) wait_vm<PWB>();
    else wait_vm<0>();
  } else {
    if (a >= A) {
      if (b > A) wait_vm<A * PWA + (A + 1) * PWB>();
      else wait_vm<A * PWA + A * PWB>();
    } else {
      wait_ab<PWA, PWB, A - 1>(a, b);
    }
  }
}

// MFMAs of one staged K-tile: A rows at sA[row * CH], W rows at sB[row * CH] (both XOR
// swizzled by row & 7, see the DMA source addresses).
// SKIP: only the wave's first fmv row fragments hold real rows (grouped experts: an expert's
// routed rows end inside the tile) — the others are neither read nor multiplied
template <class C, bool SKIP = false>
__device__ __forceinline__ void mma_tile(const bf16x8* sA, const bf16x8* sB, int lane, int wm, int wn, bool ln_acc,
                                         f32x4 (&acc)[C::FM][C::FN], float (&st_s)[C::FM], float (&st_q)[C::FM],
                                         int fmv = C::FM) {
  // All fragments of the K-tile (both 32-deep halves) are requested before the first MFMA:
  // the second half's ds_reads then complete under the first half's MFMAs instead of
  // behind an lgkmcnt(0) (the compiler counts lgkmcnt per consumer). Wave tiles with more
  // than 12 fragments per half (32 x 224: 2 + 14) load one half at a time — both halves'
  // fragments next to 28 accumulators would not fit the 256 registers of two waves per SIMD.
  constexpr bool HALVES = C::HALF_FRAGS;
  if constexpr (!HALVES) {
    bf16x8 af[2][C::FM], bw[2][C::FN];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int j = 0; j < C::FN; ++j) {
        const int row = wn * C::WTN + j * 16 + (lane & 15);
        bw[kk][j] = sB[row * C::CH + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        if (SKIP && i >= fmv) break;
        const int row = wm * C::WTM + i * 16 + (lane & 15);
        af[kk][i] = sA[row * C::CH + (chunk ^ (row & 7))];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep every ds_read ahead of the MFMAs (counted lgkmcnt waits)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (ln_acc) {
#pragma unroll
        for (int i = 0; i < C::FM; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = bf2f(af[kk][i][e]);
            st_s[i] += x;
            st_q[i] += x * x;
          }
      }
      // swapped operands: acc = (W A^T) tile, i.e. C^T — lane holds 4 consecutive output
      // COLUMNS of one row, so the epilogue moves 8-byte vectors instead of bf16 scalars
      if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        if (SKIP && i >= fmv) break;
#pragma unroll
        for (int j = 0; j < C::FN; ++j) acc[i][j] = mfma16x16x32(bw[kk][j], af[kk][i], acc[i][j]);
      }
      if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[C::FM], bw[C::FN];
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int j = 0; j < C::FN; ++j) {
        const int row = wn * C::WTN + j * 16 + (lane & 15);
        bw[j] = sB[row * C::CH + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        if (SKIP && i >= fmv) break;
        const int row = wm * C::WTM + i * 16 + (lane & 15);
        af[i] = sA[row * C::CH + (chunk ^ (row & 7))];
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ln_acc) {
#pragma unroll
        for (int i = 0; i < C::FM; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = bf2f(af[i][e]);
            st_s[i] += x;
            st_q[i] += x * x;
          }
      }
      if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        if (SKIP && i >= fmv) break;
#pragma unroll
        for (int j = 0; j < C::FN; ++j) acc[i][j] = mfma16x16x32(bw[j], af[i], acc[i][j]);
      }
      if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Joint rings (BXS == 0): A and W rows of a K-tile share one stage and one DMA batch.
// GATHER: A row r is row arows[r] of A (MoE token gather) — a compile-time switch: a runtime
// null check in every launch's prologue cost the GPT-2 GEMMs ~5 %.
// APOL: cache policy of the A rows' DMA (sc1 = 16: A was written in this launch by other
// workgroups' write-through stores — gemm_fused.hip; every other launch keeps 0)
template <class C, bool GATHER = false, int APOL = 0, int WPOL = 0>
__device__ __forceinline__ void mainloop_joint(bf16x8* smem, const bf16* __restrict__ A, int lda,
                                               const bf16* __restrict__ W, int ldw, int M, int N, int m0, int n0,
                                               int kbeg, int nk, int lane, int wave, int kgrp, int wm, int wn,
                                               bool ln_acc, f32x4 (&acc)[C::FM][C::FN], float (&st_s)[C::FM],
                                               float (&st_q)[C::FM], const int* __restrict__ arows) {
  // `wave` is the wave's index in the whole block (all K groups issue DMA); instruction
  // gi = wave*PW + j loads 8 rows of K-tile gi / INSTR of the stage
  const bf16* src[C::PW];
  int dst[C::PW];
#pragma unroll
  for (int j = 0; j < C::PW; ++j) {
    const int gi = C::EVEN ? wave * C::PW + j : min(wave * C::PW + j, C::INSTR * C::KG - 1);  // (repeats: Cfg::PW)
    const int sub = gi / C::INSTR, r8 = gi % C::INSTR;
    const int row = 8 * r8 + (lane >> 3);
    const int gch = (lane & 7) ^ (row & 7);
    const int kofs = kbeg + sub * C::BK + gch * 8;
    if (row < C::BM) {
      int gm = min(m0 + row, M - 1);
      if constexpr (GATHER) gm = arows[gm];  // gathered A rows (MoE: token of each expert-sorted row)
      src[j] = A + (size_t)gm * lda + kofs;
    } else {
      const int gn = min(n0 + row - C::BM, N - 1);
      src[j] = W + (size_t)gn * ldw + kofs;
    }
    dst[j] = sub * C::SUB + r8 * 64;
  }
  bool is_a[C::PW];  // wave-uniform: a DMA instruction covers 8 rows of one operand
#pragma unroll
  for (int j = 0; j < C::PW; ++j) {
    const int gi = C::EVEN ? wave * C::PW + j : min(wave * C::PW + j, C::INSTR * C::KG - 1);
    is_a[j] = 8 * (gi % C::INSTR) < C::BM;
  }
  auto issue = [&](int kt) {
    bf16x8* stage = smem + (kt % C::STAGES) * C::STAGE;
#pragma unroll
    for (int j = 0; j < C::PW; ++j) {
      if constexpr (APOL != 0 || WPOL != 0) {
        if (is_a[j])
          __builtin_amdgcn_global_load_lds((const void*)(src[j] + kt * (C::BK * C::KG)),
                                           (__attribute__((address_space(3))) void*)(stage + dst[j]), 16, 0, APOL);
        else
          __builtin_amdgcn_global_load_lds((const void*)(src[j] + kt * (C::BK * C::KG)),
                                           (__attribute__((address_space(3))) void*)(stage + dst[j]), 16, 0, WPOL);
        continue;
      }
      __builtin_amdgcn_global_load_lds((const void*)(src[j] + kt * (C::BK * C::KG)),
                                       (__attribute__((address_space(3))) void*)(stage + dst[j]), 16, 0, 0);
    }
  };
#pragma unroll
  for (int s = 0; s < C::STAGES - 1; ++s)
    if (s < nk) issue(s);
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = min(C::STAGES - 2, nk - 1 - kt);  // tiles issued after kt, still allowed in flight
    wait_tiles<C::PW, C::STAGES - 2>(ahead);
    raw_barrier();
    if (kt + C::STAGES - 1 < nk) issue(kt + C::STAGES - 1);
    const bf16x8* st = smem + (kt % C::STAGES) * C::STAGE + kgrp * C::SUB;
    mma_tile<C>(st, st + C::BM * C::CH, lane, wm, wn, ln_acc, acc, st_s, st_q);
  }
}

// Half-tile ring (256 x 256 tiles, 8 waves as 2 (M) x 4 (N), wave tile 128 x 64).
//
// Why: with whole 64-KiB K-tiles double-buffered (C8) the next tile is issued in one burst
// and waited for with vmcnt(0) one K-tile later; on the GPT-2 LM head every K-tile then
// stalls on the DMA (one 256-tile round of 256x256x768 tiles: 49 us = 2.1 TFLOP/s per CU,
// benchmarks/bench_lmhead.py). Here a K-tile is four 16-KiB HALF-tiles (A rows 0-127,
// A rows 128-255, W rows 0-127, W rows 128-255) in 8 slots (two K-tiles), and the wave's
// 128 x 64 output is computed as four quadrants (64 x 32, 16 MFMAs each) in the order
//   q0 (A top, W left)  q1 (A top, W right)  q2 (A bottom, W right)  q3 (A bottom, W left)
// so a K-tile's W halves are last read in q1 and its A halves in q2: K-tile t+2's W halves
// are issued into them at q2 of K-tile t and its A halves at q3 — four to six quadrant
// phases before they are read, with two to three K-tiles' worth of DMA in flight at all
// times instead of one burst per K-tile.
// Synchronisation (cdna_hip_programming.md §5, "Read a staged buffer one phase AFTER the
// wait that retires it"; RAW / WAR):
//  * q0 of K-tile t: every wave waits (counted vmcnt: only K-tile t+1's 8 DMA instructions
//    may still be outstanding) and then joins the barrier -> t's slots are complete for all;
//  * q2 / q3: a barrier before the DMA issue — every wave has finished (lgkmcnt-waited,
//    consumed by its MFMAs) the reads of the slots being re-filled (W after q1, A after q2).
// Each wave's fragment reads of a quadrant are all issued before its 16 MFMAs.
template <class C, int WPOL = 0>
__device__ __forceinline__ void mainloop_ring(bf16x8* smem, const bf16* __restrict__ A, int lda,
                                              const bf16* __restrict__ W, int ldw, int M, int N, int m0, int n0,
                                              int kbeg, int nk, int lane, int wave, int wm, int wn,
                                              f32x4 (&acc)[C::FM][C::FN]) {
  constexpr int SLOT = 128 * 8;  // bf16x8 units per 16-KiB half-tile slot (128 rows x 128 B)
  // this thread's two DMA pieces of every half-tile: rows 8 * (2 * wave + j) + lane / 8
  const bf16* srcA[2][2];
  const bf16* srcB[2][2];
  int dst[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 8 * (2 * wave + j) + (lane >> 3);
    const int gch = (lane & 7) ^ (r & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      srcA[h][j] = A + (size_t)min(m0 + h * 128 + r, M - 1) * lda + kbeg + gch * 8;
      srcB[h][j] = W + (size_t)min(n0 + h * 128 + r, N - 1) * ldw + kbeg + gch * 8;
    }
    dst[j] = (2 * wave + j) * 64;
  }
  // slot of half-tile kind hk (0 A0, 1 A1, 2 W0, 3 W1) of K-tile t
  auto slot = [&](int t, int hk) { return smem + ((t & 1) * 4 + hk) * SLOT; };
  auto issue = [&](int t, int hk) {
    const bf16* const* src = hk < 2 ? srcA[hk] : srcB[hk - 2];
    bf16x8* st = slot(t, hk);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (hk < 2)  // (hk is a literal at every call: one immediate policy per DMA)
        __builtin_amdgcn_global_load_lds((const void*)(src[j] + t * C::BK),
                                         (__attribute__((address_space(3))) void*)(st + dst[j]), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((const void*)(src[j] + t * C::BK),
                                         (__attribute__((address_space(3))) void*)(st + dst[j]), 16, 0, WPOL);
    }
  };
  // prologue: K-tiles 0 and 1 (W halves first: issue order inside a K-tile does not matter
  // for the counted waits, which retire whole K-tiles)
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (t < nk) {
      issue(t, 2);
      issue(t, 3);
      issue(t, 0);
      issue(t, 1);
    }
  const int ah = wm;            // the wave's A half (rows 128 * wm ..)
  const int bh = 2 + (wn >> 1);  // its W half
  const int brow0 = (wn & 1) * 64;
  bf16x8 af[2][4], bl[2][2], br[2][2];
  for (int t = 0; t < nk; ++t) {
    // ---- q0: K-tile t complete; A top + W left
    if (t + 1 < nk) wait_vm<8>();
    else wait_vm<0>();
    raw_barrier();
    const bf16x8* sa = slot(t, ah);
    const bf16x8* sb = slot(t, bh);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = i * 16 + (lane & 15);
        af[kk][i] = sa[row * C::CH + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = brow0 + j * 16 + (lane & 15);
        bl[kk][j] = sb[row * C::CH + (chunk ^ (row & 7))];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16x16x32(bl[kk][j], af[kk][i], acc[i][j]);
    // ---- q1: A top + W right
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = brow0 + 32 + j * 16 + (lane & 15);
        br[kk][j] = sb[row * C::CH + (chunk ^ (row & 7))];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][2 + j] = mfma16x16x32(br[kk][j], af[kk][i], acc[i][2 + j]);
    // ---- q2: every wave is past its q1 reads -> K-tile t+2's W halves go into t's W slots
    raw_barrier();
    if (t + 2 < nk) {
      issue(t + 2, 2);
      issue(t + 2, 3);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 64 + i * 16 + (lane & 15);
        af[kk][i] = sa[row * C::CH + (chunk ^ (row & 7))];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[4 + i][2 + j] = mfma16x16x32(br[kk][j], af[kk][i], acc[4 + i][2 + j]);
    // ---- q3: every wave is past its q2 reads -> K-tile t+2's A halves; A bottom + W left
    // (both already in registers)
    raw_barrier();
    if (t + 2 < nk) {
      issue(t + 2, 0);
      issue(t + 2, 1);
    }
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[4 + i][j] = mfma16x16x32(bl[kk][j], af[kk][i], acc[4 + i][j]);
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(0);
  }
}

constexpr int kPolStream = 2;  // gfx950 CPol NT (streaming) bit of the DMA's aux operand
constexpr int kPolWT = 16;     // sc1: write-through (the line leaves the XCD's L2 at the store)

// Split rings (BXS > 0): issue order B0 [A0 B1] [A1 B2] ... — iteration t issues
// A(t + SA - 1) then B(t + SB - 1). Waiting for A(t) then leaves a = min(SA-2, nk-1-t)
// later A tiles and b = min(a + 1, nk-1-t) later W tiles in flight (B(t) precedes A(t)).
template <class C, int WPOL = 0, bool SKIP = false, bool GATHER = false>
__device__ __forceinline__ void mainloop_split(bf16x8* smem, const bf16* __restrict__ A, int lda,
                                               const bf16* __restrict__ W, int ldw, int M, int N, int m0, int n0,
                                               int kbeg, int nk, int lane, int wave, int wm, int wn, bool ln_acc,
                                               f32x4 (&acc)[C::FM][C::FN], float (&st_s)[C::FM],
                                               float (&st_q)[C::FM], int fmv, const int* __restrict__ arows) {
  constexpr int D = C::SB - C::SA;  // W tiles issued ahead of the A tile of the same K step
  static_assert(D >= 1, "split rings: the W ring is deeper than the A ring");
  const bf16* srcA[C::PWA];
  const bf16* srcB[C::PWB];
  // SKIP (grouped expert launches, whose row count is the expert's, known on the device only):
  // the A rows come by buffer DMA, and a row past the expert's last one gets an offset past the
  // buffer's end — the load returns zeros WITHOUT a memory request, so the CU's LDS-DMA intake
  // carries only real rows (with clamped addresses every padding row re-read the last one).
  // Every wave still issues the same instructions: the counted vmcnt waits stay exact.
  uint32_t voffA[C::PWA];
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int j = 0; j < C::PWA; ++j) {
    const int row = 8 * (C::EVEN_A ? wave * C::PWA + j : min(wave * C::PWA + j, C::BM / 8 - 1)) + (lane >> 3);
    int gm = min(m0 + row, M - 1);
    if constexpr (GATHER) gm = arows[gm];  // gathered A rows (MoE: token of each expert-sorted row)
    srcA[j] = A + (size_t)gm * lda + kbeg + ((lane & 7) ^ (row & 7)) * 8;
    if constexpr (SKIP)
      voffA[j] = m0 + row < M ? (uint32_t)(((size_t)gm * lda + kbeg + ((lane & 7) ^ (row & 7)) * 8) * 2) : 0x80000000u;
  }
#pragma unroll
  for (int j = 0; j < C::PWB; ++j) {
    const int row = 8 * (C::EVEN_B ? wave * C::PWB + j : min(wave * C::PWB + j, C::BN / 8 - 1)) + (lane >> 3);
    const int gn = min(n0 + row, N - 1);
    srcB[j] = W + (size_t)gn * ldw + kbeg + ((lane & 7) ^ (row & 7)) * 8;
  }
  bf16x8* ringA = smem;
  bf16x8* ringB = smem + C::SA * C::A_STAGE;
  auto issueA = [&](int kt) {
    bf16x8* st = ringA + (kt % C::SA) * C::A_STAGE;
#pragma unroll
    for (int j = 0; j < C::PWA; ++j) {
      auto* dst = (__attribute__((address_space(3))) void*)(st + (C::EVEN_A ? wave * C::PWA + j : min(wave * C::PWA + j, C::BM / 8 - 1)) * 64);
      if constexpr (SKIP)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voffA[j] + kt * C::BK * 2, 0, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((const void*)(srcA[j] + kt * C::BK), dst, 16, 0, 0);
    }
  };
  auto issueB = [&](int kt) {
    bf16x8* st = ringB + (kt % C::SB) * C::B_STAGE;
#pragma unroll
    for (int j = 0; j < C::PWB; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(srcB[j] + kt * C::BK),
                                       (__attribute__((address_space(3))) void*)(st + (C::EVEN_B ? wave * C::PWB + j : min(wave * C::PWB + j, C::BN / 8 - 1)) * 64), 16,
                                       0, WPOL);
  };
  constexpr int DA = C::SA - 1;
#pragma unroll
  for (int q = 0; q < D; ++q)
    if (q < nk) issueB(q);
#pragma unroll
  for (int s = 0; s < DA; ++s) {
    if (s < nk) issueA(s);
    if (s + D < nk) issueB(s + D);
  }
  for (int kt = 0; kt < nk; ++kt) {
    const int a = min(DA - 1, nk - 1 - kt);
    // W tiles issued after A(kt): B(kt + D) .. B(min(kt + DA - 1 + D, nk - 1))
    const int b = max(0, min(DA, nk - kt - D));
    if constexpr (D == 1) wait_ab<C::PWA, C::PWB, DA - 1>(a, b);
    else wait_ab_any<C::PWA, C::PWB, DA - 1, DA>(a, b);
    raw_barrier();
    if (kt + DA < nk) issueA(kt + DA);
    if (kt + DA + D < nk) issueB(kt + DA + D);
    mma_tile<C, SKIP>(ringA + (kt % C::SA) * C::A_STAGE, ringB + (kt % C::SB) * C::B_STAGE, lane, wm, wn, ln_acc,
                      acc, st_s, st_q, fmv);
  }
}

// One output tile (tm, tn) over K-slice ks. Everything from here to the end of the epilogue
// is per tile; the kernel below maps blocks to tiles (or loops over a device-side row range).
// LN: row statistics of a folded norm accumulated in the main loop (else, with ln_mode set,
// they come from ep.ext_stats).
// WPOL: cache policy of the split rings' weight DMA (0 default, kPolStream = nt for weights
// read exactly once per step, e.g. MoE experts far larger than the MALL)
// APOL: the A rows' DMA cache policy (joint rings; mainloop_joint); PUB: the output tile is
// stored write-through (sc1) so workgroups of the SAME launch on other XCDs can read it after
// an agent-scope arrival count (gemm_fused.hip) — both 0 / false in every ordinary launch
// ONEP: the one-pass finish where the config has it (Cfg::ONE_PASS): 1 yes; 2 yes, from a kernel
// that walks several tiles (the thread <-> segment mapping is then derived again per tile: hoisted
// out of the walk its offsets stay in registers across the main loop — the row-ranged config 17
// lost a wave of occupancy, the walks of config 20 spilled 20-60 VGPRs); 0 no — the persistent
// walk of the 16-wave config 20 alone, whose kernel (128 VGPRs at most) spilled 22 VGPRs with it
// against 4 without
template <class C, int LN, int WPOL = 0, bool SKIP = false, bool GATHER = false, int APOL = 0, bool PUB = false,
          int SPOL = 0, int ONEP = 1>
__device__ __forceinline__ void glds_tile(bf16x8* smem, const bf16* __restrict__ A, int lda,
                                          const bf16* __restrict__ W, int ldw, bf16* __restrict__ Cp, int ldc,
                                          const bf16* __restrict__ bias, const bf16* __restrict__ R, int ldr,
                                          float* __restrict__ part, int M, int Mmax, int N, int K, int act,
                                          float alpha, int ks, int kslice, int tm, int tn,
                                          const float* __restrict__ ln_colsum, int ln_mode, float ln_eps,
                                          const Epi& ep, const int* __restrict__ arows = nullptr) {
  const RopeArgs& rope = ep.rope;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kgrp = wave / C::NW, wq = wave % C::NW;  // K group, wave within the group
  const int wm = wq / C::WN, wn = wq % C::WN;
  const int m0 = tm * C::BM, n0 = tn * C::BN;
  if (m0 >= M) return;  // whole block idle (uniform: before any barrier)
  DLS_STAMP(0)
  const int kbeg = ks * kslice;
  const int nk = kslice / (C::BK * C::KG);

  f32x4 acc[C::FM][C::FN];
#pragma unroll
  for (int i = 0; i < C::FM; ++i)
#pragma unroll
    for (int j = 0; j < C::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fused LayerNorm/RMSNorm prologue: row statistics of A accumulated from the A fragments
  // that stream through LDS anyway (waves with wn == 0; full K per block, splitk == 1)
  const bool ln_acc = LN && ln_mode != 0 && wn == 0;
  float st_s[C::FM], st_q[C::FM];
#pragma unroll
  for (int i = 0; i < C::FM; ++i) st_s[i] = st_q[i] = 0.f;
  if constexpr (C::RING && !SKIP && !GATHER)  // (grouped expert launches keep the joint ring)
    mainloop_ring<C, WPOL>(smem, A, lda, W, ldw, M, N, m0, n0, kbeg, nk, lane, wave, wm, wn, acc);
  else if constexpr (C::BXS > 0)
    mainloop_split<C, WPOL, SKIP, GATHER>(smem, A, lda, W, ldw, M, N, m0, n0, kbeg, nk, lane, wave, wm, wn, ln_acc, acc,
                                  st_s, st_q, min(C::FM, max(0, (M - m0 - wm * C::WTM + 15) / 16)), arows);
  else
    mainloop_joint<C, GATHER, APOL, WPOL>(smem, A, lda, W, ldw, M, N, m0, n0, kbeg, nk, lane, wave, kgrp, wm, wn, ln_acc, acc,
                                    st_s, st_q, arows);
  DLS_STAMP(1)
  const int g4 = (lane >> 4) * 4, r16 = lane & 15;
  // geometry of the staged epilogue's tile image and store pass (see below)
  constexpr int BNC = C::BN / 8;
  constexpr int BNP = BNC <= 8 ? 8 : BNC <= 16 ? 16 : BNC <= 32 ? 32 : 64;
  constexpr int NPASS = (C::BM * BNP + C::T - 1) / C::T;  // store passes of a thread
  // Batched epilogue operand requests (C::EPI_BATCH). Every global operand of the staged
  // epilogue is requested HERE, in one batch: after the K loop's final vmcnt(0) (the rings'
  // counted waits never see these loads, and nothing is live across the K loop — the operand
  // fragments are dead now), ahead of the K-group sum's barriers, so the L2 / Infinity-Cache
  // round trips run under the reduction instead of one after another behind the barriers that
  // follow. Issued before the K loop the same requests cost 2.5 % of the GPT-2 step
  // (profiles/r3_ab/gpt2_epilogue_prefetch_vs_none.txt). The loads are branch-free per lane (a
  // guarded load costs a latency each); only uniform conditions branch. They are BUFFER loads:
  // the descriptor ends with the operand, so a lane past the operand's end gets zeros without a
  // memory request (as the grouped launches' A rows, mainloop_split) — no clamp arithmetic, one
  // 32-bit offset per operand and the fragments' strides in the instructions' immediate offsets:
  // at a 1-2 us epilogue the address VALU of 64-bit clamped pointers was itself measurable.
  //  * K group 0 (it runs the image pass) asks for ext_stats of its rows and bias / ln_colsum
  //    of its columns: one 8-B / 16-B load per fragment when the operand is aligned and
  //    N % 4 == 0 (a fragment's 4 columns are then all inside N or all outside), else one
  //    clamped scalar per value, each to a register of its own (packing them would wait for
  //    every load on the spot); values of columns past N are replaced by 0 where consumed;
  //  * every thread of the store pass asks for the 16-B residual segments it will own there
  //    (rl / cc depend on tid alone); a segment that straddles N takes the scalar path below.
  const bool pre_bvec = ((reinterpret_cast<uintptr_t>(bias) & 7) | (N & 3)) == 0;
  const bool pre_cvec = ((reinterpret_cast<uintptr_t>(ln_colsum) & 15) | (N & 3)) == 0;
  // (16-B segments as in the store pass: v16 there; 32-bit byte offsets)
  const bool pre_res = C::EPI_BATCH && R != nullptr && N >= 8 && ((size_t)(M + C::BM) * ldr * 2 < (1ull << 31)) &&
                       ((reinterpret_cast<uintptr_t>(Cp) | ((uintptr_t)ldc * 2) | reinterpret_cast<uintptr_t>(R) |
                         ((uintptr_t)ldr * 2)) & 15) == 0;
  u32x2 pre_bv[C::FN];       // pre_bvec: the fragment's 4 bf16
  uint32_t pre_bs[C::FN][4];  // else: one bf16 (low half) per register
  u32x4 pre_cs[C::FN];       // fp32 bits
  u32x2 pre_st[C::FM];       // fp32 bits of (sum, sum of squares)
  u32x4 pre_r[NPASS];
  // (no initial values: a register written on the paths that request nothing would, on the
  // structurised control flow, be written behind a pending load of the other path — a wait.
  // Every read below sits under the condition its request sat under.)
  auto request_operands = [&]() {
    constexpr int kRaw = 0x00020000;  // raw buffer, 32-bit data
    if (kgrp == 0) {
      if (ln_mode != 0 && !LN) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ep.ext_stats), 0, M * 8, kRaw);
        const int vo = (m0 + wm * C::WTM + r16) * 8;  // (rows past M: zeros, never stored)
#pragma unroll
        for (int i = 0; i < C::FM; ++i) pre_st[i] = __builtin_amdgcn_raw_buffer_load_b64(rs, vo + i * 128, 0, 0);
      }
      const int c0 = n0 + wn * C::WTN + g4;  // the lane's first column; fragment j: + 16 j
      if (bias) {
        if (pre_bvec) {
          const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(bias), 0, N * 2, kRaw);
#pragma unroll
          for (int j = 0; j < C::FN; ++j) pre_bv[j] = __builtin_amdgcn_raw_buffer_load_b64(rs, c0 * 2 + j * 32, 0, 0);
        } else {
          const unsigned short* b16 = reinterpret_cast<const unsigned short*>(bias);
#pragma unroll
          for (int j = 0; j < C::FN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) pre_bs[j][e] = b16[min(c0 + j * 16 + e, N - 1)];
        }
      }
      if (ln_mode != 0) {
        if (pre_cvec) {
          const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ln_colsum), 0, N * 4, kRaw);
#pragma unroll
          for (int j = 0; j < C::FN; ++j) pre_cs[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, c0 * 4 + j * 64, 0, 0);
        } else {
          const uint32_t* c32 = reinterpret_cast<const uint32_t*>(ln_colsum);
#pragma unroll
          for (int j = 0; j < C::FN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) pre_cs[j][e] = c32[min(c0 + j * 16 + e, N - 1)];
        }
      }
    }
    if (pre_res) {
      // the descriptor ends with row M-1's N-th column: a segment of a row past M reads zeros;
      // one inside M that reaches past N reads (and nobody uses) what follows in R's buffer
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(R), 0, (int)(((size_t)(M - 1) * ldr + N) * 2), kRaw);
#pragma unroll
      for (int p = 0; p < NPASS; ++p) {
        const int q = tid + p * C::T;
        if (q < C::BM * BNP)  // (wave-uniform: BM * BNP is a multiple of 64)
          pre_r[p] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((m0 + q / BNP) * ldr + n0 + (q % BNP) * 8) * 2, 0, 0);
      }
    }
  };
  // The activation / folded-norm / RoPE choice is made ONCE per tile and the finishing pass is
  // instantiated per combination: a runtime switch per output value (apply_act) unrolled over
  // the 128 values per lane of a 256 x 256 tile compiled to ~25k instructions of branches
  // around inlined GeLU / SiLU bodies, and the instruction fetches of jumping through them made
  // this pass take 19.5 us per tile on MI355X (benchmarks/gemm_stamps.hip) — 3x the main loop
  // of the GPT-2 LM head.
  using B0 = std::integral_constant<bool, false>;
  using B1 = std::integral_constant<bool, true>;
  auto per_epilogue = [&](auto&& pass) {  // pass(act_tag, ln_tag, rope_tag)
    auto by_ln = [&](auto act_tag, auto rope_tag) {
      if (ln_mode != 0) pass(act_tag, B1{}, rope_tag);
      else pass(act_tag, B0{}, rope_tag);
    };
    if (rope.cols) {
      by_ln(std::integral_constant<int, ACT_NONE>{}, B1{});  // RoPE epilogues carry no activation
    } else {
      switch (act) {
        case ACT_GELU_TANH: by_ln(std::integral_constant<int, ACT_GELU_TANH>{}, B0{}); break;
        case ACT_SILU: by_ln(std::integral_constant<int, ACT_SILU>{}, B0{}); break;
        case ACT_RELU: by_ln(std::integral_constant<int, ACT_RELU>{}, B0{}); break;
        default: by_ln(std::integral_constant<int, ACT_NONE>{}, B0{}); break;
      }
    }
  };
  // One finished 16-byte row segment (8 bf16 of tile row rl, 16-B chunk cc) on its way out: the
  // residual add, the store, and the row statistics of what was stored. rp: the residual
  // segment as requested after the main loop (read only under pre_res). Every lane of a wave
  // calls it (the statistics' shuffles span the BNP lanes of a row).
  const bool v16 = ((reinterpret_cast<uintptr_t>(Cp) | ((uintptr_t)ldc * 2)) & 15) == 0 &&
                   (!R || ((reinterpret_cast<uintptr_t>(R) | ((uintptr_t)ldr * 2)) & 15) == 0);
  auto store_segment = [&](bf16x8 o, int rl, int cc, const u32x4& rp) {
    const int row = m0 + rl, col = n0 + cc * 8;
    float s1 = 0.f, s2 = 0.f;
    if (cc < BNC && row < M && col < N) {
      if (v16 && col + 8 <= N) {
        if (R) {
          bf16x8 r8;
          if constexpr (C::EPI_BATCH) {
            r8 = pre_res ? *reinterpret_cast<const bf16x8*>(&rp)
                         : *reinterpret_cast<const bf16x8*>(R + (size_t)row * ldr + col);
          } else {
            r8 = *reinterpret_cast<const bf16x8*>(R + (size_t)row * ldr + col);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(o[e]) + bf2f(r8[e]));
        }
        if constexpr (PUB || SPOL != 0) {  // PUB: write-through, the row segment leaves the XCD's
          // L2 for memory; SPOL: the store's cache policy (nt: streaming output)
          const auto rs = __builtin_amdgcn_make_buffer_rsrc(Cp, 0, 0x7fffffff, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&o), rs,
                                                 (int)(((size_t)row * ldc + col) * 2), 0, PUB ? 16 : SPOL);
        } else {
          *reinterpret_cast<bf16x8*>(Cp + (size_t)row * ldc + col) = o;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = bf2f(o[e]);
          s1 += y;
          s2 += y * y;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (col + e >= N) continue;
          float x = bf2f(o[e]);
          if (R) x += bf2f(R[(size_t)row * ldr + col + e]);
          const bf16 ob = f2bf(x);
          Cp[(size_t)row * ldc + col + e] = ob;
          const float y = bf2f(ob);
          s1 += y;
          s2 += y * y;
        }
      }
    }
    if (ep.stats_out) {
#pragma unroll
      for (int o_ = 1; o_ < BNP; o_ <<= 1) {
        s1 += __shfl_xor(s1, o_, 64);
        s2 += __shfl_xor(s2, o_, 64);
      }
      if (cc == 0 && row < M) {
        atomicAdd(ep.stats_out + 2 * row, s1);
        atomicAdd(ep.stats_out + 2 * row + 1, s2);
      }
    }
  };
  if constexpr (C::ONE_PASS && ONEP != 0) {
    // One-pass finish (Cfg::ONE_PASS). A split-K slice (partial store or in-launch combine) and
    // SwiGLU return before the staged epilogue and keep the K-group sum below.
    static_assert(!LN, "K-grouped tiles take no in-kernel row statistics (launch_gemm_glds)");
    static_assert(BNP == 8 && C::BM * BNP <= C::T && (C::BM * BNP) % 64 == 0,
                  "one 16-B segment per thread, 8 lanes per tile row, whole waves");
    if (part == nullptr && act != ACT_SWIGLU) {
      // Thread tid < BM * 8 owns chunk cc = tid % 8 (columns 8cc .. 8cc+7) of tile row
      // rl = tid / 8 — the store pass's mapping; the waves past BM * 8 (config 45: 5 of 8, config
      // 20: 8 of 16) only hand their fragments over. All operands of the segment are requested
      // here, in one batch, as request_operands does for the staged epilogue: range-checked
      // buffer loads (rows past M and, with the vector forms, columns past N read zeros), no
      // barrier between here and their use waits on vmcnt.
      int tid1 = tid;
      if constexpr (ONEP == 2) asm volatile("" : "+v"(tid1));  // (tile walks: derived HERE, per tile)
      const int lane1 = tid1 & 63, kgrp1 = (tid1 >> 6) / C::NW, wq1 = (tid1 >> 6) % C::NW, wn1 = wq1 % C::WN;
      const bool own = tid1 < C::BM * BNP;  // (wave-uniform)
      const int rl = tid1 / BNP, cc = tid1 % BNP;
      const int row = m0 + rl, col = n0 + cc * 8;
      u32x2 o_st;        // fp32 bits of the row's (sum, sum of squares)
      u32x2 o_bv[2];     // pre_bvec: 4 bf16 each
      uint32_t o_bs[8];  // else: one bf16 (low half) per register
      u32x4 o_cs[2];     // fp32 bits
      u32x4 o_r;
      if (own) {
        constexpr int kRaw = 0x00020000;  // raw buffer, 32-bit data
        if (ln_mode != 0) {
          const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ep.ext_stats), 0, M * 8, kRaw);
          o_st = __builtin_amdgcn_raw_buffer_load_b64(rs, row * 8, 0, 0);
        }
        if (bias) {
          if (pre_bvec) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(bias), 0, N * 2, kRaw);
#pragma unroll
            for (int h = 0; h < 2; ++h) o_bv[h] = __builtin_amdgcn_raw_buffer_load_b64(rs, col * 2 + h * 8, 0, 0);
          } else {
            const unsigned short* b16 = reinterpret_cast<const unsigned short*>(bias);
#pragma unroll
            for (int e = 0; e < 8; ++e) o_bs[e] = b16[min(col + e, N - 1)];
          }
        }
        if (ln_mode != 0) {
          if (pre_cvec) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ln_colsum), 0, N * 4, kRaw);
#pragma unroll
            for (int h = 0; h < 2; ++h) o_cs[h] = __builtin_amdgcn_raw_buffer_load_b128(rs, col * 4 + h * 16, 0, 0);
          } else {
            const uint32_t* c32 = reinterpret_cast<const uint32_t*>(ln_colsum);
#pragma unroll
            for (int e = 0; e < 8; ++e) o_cs[e >> 2][e & 3] = c32[min(col + e, N - 1)];
          }
        }
        if (pre_res) {
          // (the descriptor ends with row M-1's N-th column, as in request_operands)
          const auto rs =
              __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(R), 0, (int)(((size_t)(M - 1) * ldr + N) * 2), kRaw);
          o_r = __builtin_amdgcn_raw_buffer_load_b128(rs, (row * ldr + col) * 2, 0, 0);
        }
      }
      // Fragment regions: K group g owns REG f32x4 records at red + g * REG; the record of
      // fragment (i, j) of wave wq = wm * WN + wn and lane (g4i = lane >> 4, r16 = lane & 15) —
      // row wm * WTM + 16 i + r16, columns cl .. cl + 3, cl = wn * WTN + 16 j + 4 g4i — sits at
      //   ((i * FN + j) * NW + wq) * 64 + 16 * g4i + (r16 ^ (((cl >> 3) & 3) << 2)).
      // Write side: 8 consecutive lanes share g4i, so the XOR permutes them inside their own 8
      // records (128 B): every ds_write_b128 group covers the 32 write banks once. Read side: the
      // 16 lanes of a ds_read_b128 group are 4 consecutive chunks cc of each of 4 tile rows whose
      // r16 differ in bits 0-1 only; record index mod 16 (the 16-B slot of the 256-B bank row)
      // is r16 ^ ((cc & 3) << 2) — 16 different slots, conflict-free (unswizzled: 4-way). The two
      // records of a segment (columns 8cc .. +3 and +4 .. +7: g4i and g4i + 1) are 16 apart.
      constexpr int REG = C::NW * C::FM * C::FN * 64;
      f32x4* red = reinterpret_cast<f32x4*>(smem);
      epi_barrier<true>();  // every wave is done with the staging buffers
#pragma unroll
      for (int i = 0; i < C::FM; ++i)
#pragma unroll
        for (int j = 0; j < C::FN; ++j) {
          const int cl = wn1 * C::WTN + j * 16 + (lane1 >> 4) * 4;
          red[kgrp1 * REG + ((i * C::FN + j) * C::NW + wq1) * 64 + (lane1 & 48) +
              ((lane1 & 15) ^ (((cl >> 3) & 3) << 2))] = acc[i][j];
        }
      epi_barrier<true>();  // every group's fragments are in LDS (the operand requests stay in flight)
      DLS_STAMP(7)
      if (own) {
        // (chunks past the tile's BNC — 48-column tiles — read chunk BNC - 1 again and store nothing)
        const int ccr = min(cc, BNC - 1), cl0 = ccr * 8;
        const int rec = (((rl % C::WTM) / 16 * C::FN + (cl0 % C::WTN) / 16) * C::NW + (rl / C::WTM) * C::WN +
                         cl0 / C::WTN) * 64 + (cl0 & 8) * 4 + ((rl & 15) ^ ((ccr & 3) << 2));
        f32x4 part_lo[C::KG], part_hi[C::KG];
#pragma unroll
        for (int g2 = 0; g2 < C::KG; ++g2) {
          part_lo[g2] = red[g2 * REG + rec];
          part_hi[g2] = red[g2 * REG + rec + 16];
        }
        // the K groups' sum in the order ((g0 + g1) + g2) + g3, as group 0 added them
        f32x4 lo = part_lo[0], hi = part_hi[0];
#pragma unroll
        for (int g2 = 1; g2 < C::KG; ++g2) {
          lo += part_lo[g2];
          hi += part_hi[g2];
        }
        float ln_rs1 = 0.f, ln_mu1 = 0.f;
        if (ln_mode != 0) {
          const float inv_k = 1.0f / (float)K;
          consume_from_here(o_st);
          const float a = __uint_as_float(o_st[0]), q = __uint_as_float(o_st[1]);
          const float mu = ln_mode == 1 ? a * inv_k : 0.f;
          ln_mu1 = mu;
          ln_rs1 = rsqrtf(fmaxf(q * inv_k - mu * mu, 0.f) + ln_eps);
        }
        bf16x8 o;
        auto finish = [&](auto act_tag, auto ln_tag, auto rope_tag) {
          constexpr int ACT = decltype(act_tag)::value;
          constexpr bool LNM = decltype(ln_tag)::value, ROPE = decltype(rope_tag)::value;
          float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          float csv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // colsum(W') of the 8 columns (folded norm)
          if (bias) {
            uint32_t w[8];  // (a bf16 is the high half of its fp32)
            if (pre_bvec) {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                consume_from_here(o_bv[h]);
                const uint32_t p0 = o_bv[h][0], p1 = o_bv[h][1];
                w[4 * h + 0] = p0 << 16;
                w[4 * h + 1] = p0 & 0xffff0000u;
                w[4 * h + 2] = p1 << 16;
                w[4 * h + 3] = p1 & 0xffff0000u;
              }
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                consume_from_here(o_bs[e]);
                w[e] = o_bs[e] << 16;
              }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) bv[e] = col + e < N ? __uint_as_float(w[e]) : 0.f;
          }
          if constexpr (LNM) {
#pragma unroll
            for (int h = 0; h < 2; ++h) consume_from_here(o_cs[h]);
#pragma unroll
            for (int e = 0; e < 8; ++e) csv[e] = col + e < N ? __uint_as_float(o_cs[e >> 2][e & 3]) : 0.f;
          }
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = e < 4 ? lo[e & 3] : hi[e & 3];
            v[e] = finish_value<ACT, LNM>(x, alpha, ln_rs1, ln_mu1, csv[e], bv[e]);
          }
          if constexpr (ROPE) {
            rope_pairs<4>(v, row, col, rope);
            rope_pairs<4>(v + 4, row, col + 4, rope);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
        };
        per_epilogue(finish);
        if (pre_res) consume_from_here(o_r);
        store_segment(o, rl, cc, o_r);
      }
      DLS_STAMP(3)
      return;
    }
  }
  if constexpr (C::EPI_BATCH) {
    // (a split-K slice stores a partial tile, and SwiGLU has its own epilogue: neither reaches
    // the staged epilogue; the in-launch combine asks once it knows it is the last arriver)
    if (part == nullptr && act != ACT_SWIGLU) request_operands();
  }
  if constexpr (C::KG > 2) {
    // sum the K groups' accumulators into group 0 in ONE round: group g >= 1 writes its
    // fragments to its own region of the (now free) staging buffers, one barrier, and group 0
    // adds the regions in the order 1, 2, .., KG-1 — the same sum, bit for bit, as a write /
    // barrier / add / barrier round per group. The staged epilogue's own barrier (or the norm
    // statistics' / the split-K combine's) separates group 0's reads from the next LDS writes.
    constexpr int REG = C::NW * C::FM * C::FN * 64;  // f32x4 records per group
    epi_barrier<C::EPI_BATCH>();  // every wave is done with the staging buffers
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    if (kgrp != 0) {
#pragma unroll
      for (int i = 0; i < C::FM; ++i)
#pragma unroll
        for (int j = 0; j < C::FN; ++j)
          red[(kgrp - 1) * REG + ((i * C::FN + j) * C::NW + wq) * 64 + lane] = acc[i][j];
    }
    epi_barrier<C::EPI_BATCH>();
    if (kgrp == 0) {
#pragma unroll
      for (int g2 = 1; g2 < C::KG; ++g2)
#pragma unroll
        for (int i = 0; i < C::FM; ++i)
#pragma unroll
          for (int j = 0; j < C::FN; ++j)
            acc[i][j] += red[(g2 - 1) * REG + ((i * C::FN + j) * C::NW + wq) * 64 + lane];
    }
  } else if constexpr (C::KG > 1) {
    // sum the K groups' accumulators into group 0 (lane-contiguous 16-B records)
    epi_barrier<C::EPI_BATCH>();
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    for (int g2 = 1; g2 < C::KG; ++g2) {
      if (kgrp == g2) {
#pragma unroll
        for (int i = 0; i < C::FM; ++i)
#pragma unroll
          for (int j = 0; j < C::FN; ++j) red[((i * C::FN + j) * C::NW + wq) * 64 + lane] = acc[i][j];
      }
      epi_barrier<C::EPI_BATCH>();
      if (kgrp == 0) {
#pragma unroll
        for (int i = 0; i < C::FM; ++i)
#pragma unroll
          for (int j = 0; j < C::FN; ++j) acc[i][j] += red[((i * C::FN + j) * C::NW + wq) * 64 + lane];
      }
      epi_barrier<C::EPI_BATCH>();
    }
  }

  DLS_STAMP(7)
  if (part != nullptr && ep.tile_sem != nullptr) {
    // In-launch split-K combine (cdna_hip_programming.md §projection GEMM item 2, sc1 form):
    // every K slice stores its fp32 tile WRITE-THROUGH (sc1) into its slab, drains, and one
    // lane draws a ticket from the tile's agent-scope counter; the slice that draws
    // splitk-1 reads the other slabs with sc1 loads (no L1 copy can be stale), adds them to
    // its registers and runs the ordinary epilogue. No separate reduce kernel, no spinning.
    const size_t slab = (size_t)Mmax * N;
    const int tiles_m = (M + C::BM - 1) / C::BM;
    int* sem = ep.tile_sem + tm + tn * tiles_m;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(part, 0, (int)(slab * kslice_count(K, kslice) * 4), 0x00020000);
    if (kgrp == 0) {
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        const int row = m0 + wm * C::WTM + i * 16 + r16;
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < C::FN; ++j) {
          const int col = n0 + wn * C::WTN + j * 16 + g4;
          if (col >= N) continue;  // N % 8 == 0 on split-K launches: a fragment is in or out whole
          const f32x4 v = acc[i][j];
          u32x4 u = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
          __builtin_amdgcn_raw_buffer_store_b128(u, rsrc, (int)(((size_t)ks * slab + (size_t)row * N + col) * 4), 0,
                                                 16);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem);  // the block's one LDS array (staging is free now)
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(sem, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == kslice_count(K, kslice) - 1;
      if (last) __hip_atomic_store(sem, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
      flag[0] = last;
    }
    __syncthreads();
    const bool last = flag[0] != 0;
    if (!last) return;  // block-uniform
    if constexpr (C::EPI_BATCH) {
      if (act != ACT_SWIGLU) request_operands();  // the last arriver runs the staged epilogue
    }
    if (kgrp == 0) {
      const int nsl = kslice_count(K, kslice);
      for (int s2 = 0; s2 < nsl; ++s2) {
        if (s2 == ks) continue;
#pragma unroll
        for (int i = 0; i < C::FM; ++i) {
          const int row = min(m0 + wm * C::WTM + i * 16 + r16, M - 1);
#pragma unroll
          for (int j = 0; j < C::FN; ++j) {
            const int col = min(n0 + wn * C::WTN + j * 16 + g4, N - 4);
            const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(
                rsrc, (int)(((size_t)s2 * slab + (size_t)row * N + col) * 4), 0, 16);
            acc[i][j] += f32x4{__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]),
                               __uint_as_float(u[3])};
          }
        }
      }
    }
    part = nullptr;  // the tile now holds the full sum: ordinary epilogue below
  }
  // epilogue: lane (g = lane>>4, r = lane&15) of fragment (i, j) holds C[row][col..col+3]
  // with row = m0 + wm*WTM + 16i + r, col = n0 + wn*WTN + 16j + 4g
  float ln_rs[C::FM], ln_mu[C::FM];
  if (ln_mode != 0) {
    if constexpr (LN) {
    // reduce the 4 lane groups (k-chunks) -> full-row sums, publish per row via LDS
    float* stats = reinterpret_cast<float*>(smem);
    raw_barrier();  // every wave is past its last LDS read of the staging buffers
    if (ln_acc) {
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        float a = st_s[i], q = st_q[i];
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        if (lane < 16) {
          const int lr = wm * C::WTM + i * 16 + lane;
          stats[2 * lr] = a;
          stats[2 * lr + 1] = q;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < C::FM; ++i) {
      const int lr = wm * C::WTM + i * 16 + r16;
      const float a = stats[2 * lr], q = stats[2 * lr + 1];
      const float inv_k = 1.0f / (float)K;
      if (ln_mode == 1) {
        const float mu = a * inv_k;
        const float var = fmaxf(q * inv_k - mu * mu, 0.f);
        ln_mu[i] = mu;
        ln_rs[i] = rsqrtf(var + ln_eps);
      } else {
        ln_mu[i] = 0.f;
        ln_rs[i] = rsqrtf(q * inv_k + ln_eps);
      }
    }
      } else {
      // statistics handed over by the producer of A (fp32 [M][2] = sum, sum of squares)
      const float inv_k = 1.0f / (float)K;
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        float a, q;
        if (C::EPI_BATCH && act != ACT_SWIGLU) {  // requested after the main loop by K group 0 (the others' are unused)
          a = q = 0.f;
          if (kgrp == 0) {
            consume_from_here(pre_st[i]);
            a = __uint_as_float(pre_st[i][0]);
            q = __uint_as_float(pre_st[i][1]);
          }
        } else {
          const int row = min(m0 + wm * C::WTM + i * 16 + r16, M - 1);
          a = ep.ext_stats[2 * row];
          q = ep.ext_stats[2 * row + 1];
        }
        const float mu = ln_mode == 1 ? a * inv_k : 0.f;
        ln_mu[i] = mu;
        ln_rs[i] = rsqrtf(fmaxf(q * inv_k - mu * mu, 0.f) + ln_eps);
      }
    }
  }
  // 8-byte vector stores need 8-B aligned rows (ldc % 4 == 0) — N itself may be ragged
  // (the LM head writes 50257 columns into rows padded to 50304); a fragment whose 4
  // columns straddle N falls back to scalars.
  const bool vec_ok = (ldc % 4 == 0) && (!R || ldr % 4 == 0);
  if (part != nullptr) {  // split-K: fp32 partial slab, reduced by splitk_reduce_kernel
    if (kgrp != 0) return;
    float* P = part + (size_t)ks * Mmax * N;
#pragma unroll
    for (int i = 0; i < C::FM; ++i) {
      const int row = m0 + wm * C::WTM + i * 16 + r16;
      if (row >= M) continue;
#pragma unroll
      for (int j = 0; j < C::FN; ++j) {
        const int col = n0 + wn * C::WTN + j * 16 + g4;
        if (N % 4 == 0 && col + 3 < N) {
          const f32x4 v = acc[i][j];
          store16_pol<SPOL>(P, ((size_t)row * N + col) * 4,
                            u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]),
                                  __float_as_uint(v[3])});
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < N) P[(size_t)row * N + col + e] = acc[i][j][e];
        }
      }
    }
    return;
  }
  if (act == ACT_SWIGLU) {
    if (kgrp != 0) return;
    // fragment pairs (2jj, 2jj+1) hold gate and up for the same 16 output columns
    const int NO = N / 2;
#pragma unroll
    for (int jj = 0; jj < C::FN / 2; ++jj) {
      const int gcol = n0 + wn * C::WTN + jj * 32 + g4;  // gate column in W' space
      const int ocol = (n0 + wn * C::WTN) / 2 + jj * 16 + g4;
      if (ocol >= NO) continue;
      float bg[4] = {0.f, 0.f, 0.f, 0.f}, bu[4] = {0.f, 0.f, 0.f, 0.f};
      float cg[4] = {0.f, 0.f, 0.f, 0.f}, cu[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (bias) {
          bg[e] = bf2f(bias[gcol + e]);
          bu[e] = bf2f(bias[gcol + 16 + e]);
        }
        if (ln_mode != 0) {
          cg[e] = ln_colsum[gcol + e];
          cu[e] = ln_colsum[gcol + 16 + e];
        }
      }
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        const int row = m0 + wm * C::WTM + i * 16 + r16;
        if (row >= M) continue;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float g = acc[i][2 * jj][e], u = acc[i][2 * jj + 1][e];
          if (ln_mode != 0) {
            g = ln_rs[i] * (g - ln_mu[i] * cg[e]);
            u = ln_rs[i] * (u - ln_mu[i] * cu[e]);
          } else {
            g *= alpha;
            u *= alpha;
          }
          o[e] = f2bf(silu(g + bg[e]) * (u + bu[e]));
        }
        if (vec_ok && ocol + 3 < NO) {
          store8_pol<SPOL>(Cp, ((size_t)row * ldc + ocol) * 2, *reinterpret_cast<const u32x2*>(&o));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (ocol + e < NO) Cp[(size_t)row * ldc + ocol + e] = o[e];
        }
      }
    }
    return;
  }
  // Staged epilogue: each wave writes its finished fragments (bias, activation, folded norm,
  // RoPE applied; bf16) into a tile image in LDS, then the block stores the tile as whole
  // 16-B-per-lane row segments (residual add and row statistics on the way out). A lane's
  // fragment holds only 4 columns (8 B) of 16 different rows, so storing fragments directly
  // scatters 32-B pieces over 16 rows per instruction — partial lines that measured
  // ~1.2 TB/s on the 51 MB LM-head output; full rows run at the HBM write rate.
  // BNC 16-B chunks per tile row, stored in rows of BNP (power of two >= 8) chunks: image chunk
  // c of row r sits at c ^ (r & 7), and BNP consecutive lanes own one row in the store pass
  static_assert(C::BN % 8 == 0 && BNC <= 64, "staged epilogue: BN % 8 == 0, BN <= 512");
  static_assert(C::BM * BNP * 16 <= C::LDS_UNITS * 16, "output tile image must fit the staging LDS");
  static_assert((C::BM * BNP) % 64 == 0 && ((C::BM * BNP) % C::T == 0 || C::BM * BNP < C::T),
                "store pass: every wave makes the same number of passes (shuffles stay wave-uniform)");
  bf16* img = reinterpret_cast<bf16*>(smem);
  epi_barrier<C::EPI_BATCH>();  // every wave is done with the staging buffers (and the norm statistics)
  // (one instance of the fragment pass per activation / folded-norm / RoPE choice: per_epilogue)
  auto image_pass = [&](auto act_tag, auto ln_tag, auto rope_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    constexpr bool LNM = decltype(ln_tag)::value, ROPE = decltype(rope_tag)::value;
#pragma unroll
    for (int j = 0; j < C::FN; ++j) {
      if (kgrp != 0) break;  // K group 0 holds the summed tile
      const int cl = wn * C::WTN + j * 16 + g4;  // local column of this lane's 4 values
      const int col = n0 + cl;
      const bool full = col + 3 < N;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      float csv[4] = {0.f, 0.f, 0.f, 0.f};  // colsum(W') of the 4 columns (folded norm)
      if constexpr (C::EPI_BATCH) {
        // requested after the main loop from clamped addresses: a column past N reads as 0
        if (bias) {
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[e] = 0.f;
          uint32_t w[4];  // (a bf16 is the high half of its fp32)
          if (pre_bvec) {
            consume_from_here(pre_bv[j]);
            const uint32_t p0 = pre_bv[j][0], p1 = pre_bv[j][1];
            w[0] = p0 << 16;
            w[1] = p0 & 0xffff0000u;
            w[2] = p1 << 16;
            w[3] = p1 & 0xffff0000u;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              consume_from_here(pre_bs[j][e]);
              w[e] = pre_bs[j][e] << 16;
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[e] = col + e < N ? __uint_as_float(w[e]) : 0.f;
        }
        if constexpr (LNM) {
          consume_from_here(pre_cs[j]);
#pragma unroll
          for (int e = 0; e < 4; ++e) csv[e] = col + e < N ? __uint_as_float(pre_cs[j][e]) : 0.f;
        }
        (void)full;
      } else {
      if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = col + e < N ? bf2f(bias[col + e]) : 0.f;
      }
      if constexpr (LNM) {
        if (full && (N % 4 == 0)) {
          const f32x4 c4 = *reinterpret_cast<const f32x4*>(ln_colsum + col);
#pragma unroll
          for (int e = 0; e < 4; ++e) csv[e] = c4[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) csv[e] = col + e < N ? ln_colsum[col + e] : 0.f;
        }
      }
      }
#pragma unroll
      for (int i = 0; i < C::FM; ++i) {
        const int rl = wm * C::WTM + i * 16 + r16;
        float v[4];
        if constexpr (LNM) {
          // W.LN(x) = rstd * (W' x - mu * colsum(W')) + (bias + W b), W' = W * ln_w (host-derived)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = act_c<ACT>(ln_rs[i] * (acc[i][j][e] - ln_mu[i] * csv[e]) + bv[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = act_c<ACT>(alpha * acc[i][j][e] + bv[e]);
        }
        if constexpr (ROPE) rope_pairs<4>(v, m0 + rl, col, rope);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
        *reinterpret_cast<bf16x4*>(img + rl * BNP * 8 + (((cl >> 3) ^ (rl & 7)) << 3) + (cl & 7)) = o;
      }
    }
  };
  per_epilogue(image_pass);
  epi_barrier<C::EPI_BATCH>();  // the image is complete (the residual requests stay in flight)
  DLS_STAMP(2)
  if constexpr (C::EPI_BATCH) {
    if (pre_res) {
#pragma unroll
      for (int p = 0; p < NPASS; ++p)
        if (tid + p * C::T < C::BM * BNP) consume_from_here(pre_r[p]);
    }
  }
  const bf16x8* img8 = reinterpret_cast<const bf16x8*>(img);
  const int tid_ = threadIdx.x;
  // consecutive groups of BNP threads own one tile row per pass (lanes past BNC idle)
#pragma unroll 2
  for (int q = tid_; q < C::BM * BNP; q += C::T) {
    const int rl = q / BNP, cc = q % BNP;
    // the residual segment as requested after the main loop (pass q / T of this thread)
    u32x4 rp;
    if constexpr (C::EPI_BATCH) {
      rp = pre_r[0];
#pragma unroll
      for (int p = 1; p < NPASS; ++p) rp = q / C::T == p ? pre_r[p] : rp;
    }
    store_segment(img8[rl * BNP + (cc ^ (rl & 7))], rl, cc, rp);
  }
  DLS_STAMP(3)
}

// LN / RANGED are compile-time switches: a kernel instance carries only the epilogue and
// tile walk it needs (the folded-norm statistics and the row-range loop cost registers).
// POL (plain tiles only): streaming (nt) cache policy of the weight DMA (bit 0, split rings)
// and of the output stores (bit 1) — GemmArgs::stream_pol
// Grouped expert launches: a TALLER tile of the same column width that takes an expert whose
// routed rows overflow C's tile but fit this one in ONE pass over its weight panel (instead of
// a partner block streaming the whole panel again for a few rows). void: none. Specialised
// below the tile configs; enabled by w_stream bit 256 (DLS_EXPERT_TALL).
template <class C>
struct TallTile {
  using type = void;
};
template <class C>
constexpr int tall_lds_units() {
  if constexpr (std::is_void_v<typename TallTile<C>::type>) return 0;
  else return TallTile<C>::type::LDS_UNITS;
}

template <class C, int LN, int RANGED, int POL = 0>
__global__ __launch_bounds__(C::T, C::OCC) void gemm_glds_kernel(const bf16* __restrict__ A, int lda,
                                                         const bf16* __restrict__ W, int ldw, bf16* __restrict__ Cp,
                                                         int ldc, const bf16* __restrict__ bias,
                                                         const bf16* __restrict__ R, int ldr,
                                                         float* __restrict__ part, int M, int N, int K, int act,
                                                         float alpha, int tiles_m, int tiles_n, int splitk,
                                                         int kslice, const float* __restrict__ ln_colsum,
                                                         int ln_mode, float ln_eps, const int* __restrict__ rows,
                                                         int compact_rows, Epi ep) {
  constexpr int kUnits = RANGED == 3 && tall_lds_units<C>() > C::LDS_UNITS ? tall_lds_units<C>() : C::LDS_UNITS;
  __shared__ bf16x8 smem[kUnits];
  const int ntile = tiles_m * tiles_n;
  if constexpr (RANGED == 2) {
    // persistent: a resident grid walks the tiles; tile t+1's first K-tiles are issued right
    // behind tile t's epilogue stores, so the store drain overlaps the next load latency
    // instead of holding the CU (one block per CU cannot overlap them across blocks)
    const int total = ntile * splitk;
    for (int L = blockIdx.x, it = 0; L < total; L += gridDim.x, ++it) {
      // every wave is done reading the previous tile's output image (one-pass configs: the K
      // groups' fragment regions) — the next tile's DMA refills the same staging buffers
      if (it) raw_barrier();
      const int ks = L / ntile, tile = L % ntile;
      glds_tile<C, LN, 0, false, false, 0, false, 0, (C::T <= 512 ? 2 : 0)>(smem, A, lda, W, ldw, Cp, ldc, bias, R, ldr, part, M, M, N, K, act, alpha, ks, kslice,
                       tile % tiles_m, tile / tiles_m, ln_colsum, (LN || ep.ext_stats) ? ln_mode : 0, ln_eps, ep);
    }
    return;
  }
  if constexpr (RANGED == 3) {
    // grouped MoE experts: block (g, tn) walks expert g's row range [rows[g], rows[g+1]) of
    // its column panel with expert g's weight; consecutive blocks share an expert (its rows
    // stay L2-resident while its weight panels stream)
    // (w_stream bit 8: groups sharing weights — panel-major, the panel's groups on one XCD)
    // (w_stream bit 16: row-split PAIRS — blocks b and b + 8 of each 16 sit on the same XCD and
    // start together; the pair splits (g, tn)'s row tiles even / odd, so an expert with more routed
    // rows than one tile streams its weight panel from HBM once, the partner's copy from the L2,
    // instead of a second serial pass re-streaming it: profiles/r6_mixtral/rows_vs_time.txt. The
    // odd partner of an expert that fits one tile exits at once)
    int g = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n, t0 = 0, dt = 1;
    if (ep.w_stream & 8) {
      const int L = xcd_remap(blockIdx.x, gridDim.x), ng = gridDim.x / tiles_n;
      tn = L / ng;
      g = L % ng;
    } else if (ep.w_stream & 16) {
      const int pair = (blockIdx.x >> 4) * 8 + (blockIdx.x & 7);
      if (pair >= tiles_m * tiles_n) return;  // grid rounded up to whole 16-block groups
      g = pair / tiles_n;
      tn = pair % tiles_n;
      t0 = (blockIdx.x >> 3) & 1;
      dt = 2;
    } else if (ep.w_stream & (32 | 64)) {
      // the odd partners as one half of the grid: dispatched after every even block (bit 32) or
      // before them (bit 64). A heavy expert's second row tile then runs on a CU of its own, in
      // parallel with its first, where the serial walk doubled its blocks' time: Mixtral-8x7B
      // 24.74 -> 23.58 ms per step (profiles/r6_ab/expert_pairs.txt)
      const int half = gridDim.x >> 1, second = blockIdx.x >= half, idx = blockIdx.x - second * half;
      t0 = second == ((ep.w_stream & 32) != 0);
      dt = 2;
      g = idx / tiles_n;
      tn = idx % tiles_n;
    }
    if ((ep.w_stream & 128) && !(ep.w_stream & (8 | 16))) {
      // XCD-affine walk (w_stream bit 128): blocks on XCD x (index % 8 under round-robin
      // dispatch) take a CONTIGUOUS run of the (group, column panel) order, so an XCD works
      // through one expert's panels at a time and that expert's rows stay in ITS L2 — the
      // plain order spreads every expert's blocks over all eight XCDs, and each L2 then holds
      // all eight experts' rows (Mixtral down: 8 x 3.7 MB against a 4 MB L2)
      const int total = tiles_m * tiles_n, idx = g * tiles_n + tn;
      const int x = idx & 7, j = idx >> 3, q = total >> 3, r = total & 7;
      const int L = x * q + min(x, r) + j;
      g = L / tiles_n;
      tn = L % tiles_n;
    }
    const int r0 = rows[g], cnt = rows[g + 1] - r0;
    const int Mr = compact_rows ? min(cnt, compact_rows) : cnt;
    const bf16* Wg = reinterpret_cast<const bf16*>(ep.grp_w[g]);
    bf16* Cg = ep.grp_c ? reinterpret_cast<bf16*>(ep.grp_c[g]) : Cp + (size_t)r0 * ldc;
    // gathered A: the group's rows are tokens a_rows[r0 ..]; else rows r0.. of the sorted A.
    // The gather map travels in the `part` argument, unused by grouped launches (no split-K):
    // a new Epi field would change every GEMM launch's argument layout
    const int* a_rows = reinterpret_cast<const int*>(part);
    const int* ag = a_rows ? a_rows + r0 : nullptr;
    const bf16* Ag = a_rows ? A : A + (size_t)r0 * lda;
    if constexpr (!std::is_void_v<typename TallTile<C>::type>) {
      // SPLIT = 2: the taller tile is half as wide — the block and its partner each take one half
      // of the column panel over ALL of the expert's rows (each streams half the panel once; in
      // the serial walk without partners the block takes both halves in turn)
      using T2 = typename TallTile<C>::type;
      constexpr int SPLIT = C::BN / T2::BN;
      static_assert((SPLIT == 1 || SPLIT == 2) && T2::BN * SPLIT == C::BN && T2::BM > C::BM && T2::T == C::T,
                    "a taller tile of the same panel (or of half of it)");
      if ((ep.w_stream & 256) && Mr > C::BM && Mr <= T2::BM) {
        const bool nt = T2::BXS > 0 && (ep.w_stream & 1);
        for (int hh = t0; hh < SPLIT; hh += dt) {  // (SPLIT 1: a partner block has nothing to do)
          if (hh != t0) raw_barrier();
          const int tn2 = tn * SPLIT + hh;
          if (a_rows) {
            if (nt)
              glds_tile<T2, 0, kPolStream, true, true>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0, nullptr, Mr,
                                                       M, N, K, act, alpha, 0, K, 0, tn2, ln_colsum, 0, ln_eps, ep, ag);
            else
              glds_tile<T2, 0, 0, false, true>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0, nullptr, Mr, M, N,
                                               K, act, alpha, 0, K, 0, tn2, ln_colsum, 0, ln_eps, ep, ag);
          } else {
            if (nt)
              glds_tile<T2, 0, kPolStream, true, false>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0, nullptr,
                                                        Mr, M, N, K, act, alpha, 0, K, 0, tn2, ln_colsum, 0, ln_eps, ep,
                                                        ag);
            else
              glds_tile<T2, 0, 0, false, false>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0, nullptr, Mr, M, N,
                                                K, act, alpha, 0, K, 0, tn2, ln_colsum, 0, ln_eps, ep, ag);
          }
        }
        return;
      }
    }
#define DLS_GROUPED_WALK(GA)                                                                                      \
  for (int t = t0; t * C::BM < Mr; t += dt) {                                                                      \
    if (t != t0) raw_barrier(); /* every wave is done reading the staging buffers of the previous tile */          \
    if (C::BXS > 0 && (ep.w_stream & 1))                                                                           \
      glds_tile<C, 0, kPolStream, true, GA, 0, false, 0, 2>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0,     \
                                                            nullptr, Mr, M, N, K, act, alpha, 0, K, t, tn,        \
                                                            ln_colsum, 0, ln_eps, ep, ag);                        \
    else                                                                                                           \
      glds_tile<C, 0, 0, false, GA, 0, false, 0, 2>(smem, Ag, lda, Wg, ldw, Cg, ldc, bias, nullptr, 0, nullptr,    \
                                                    Mr, M, N, K, act, alpha, 0, K, t, tn, ln_colsum, 0, ln_eps,   \
                                                    ep, ag);                                                       \
  }
    if (a_rows) {
      DLS_GROUPED_WALK(true)
    } else {
      DLS_GROUPED_WALK(false)
    }
#undef DLS_GROUPED_WALK
    return;
  }
  const int bid = xcd_remap(blockIdx.x, ntile * splitk);
  int ks = bid / ntile, tile = bid % ntile;
  int tm = tile % tiles_m, tn = tile / tiles_m;
  if constexpr (!RANGED) {
    if (compact_rows > 0) {
      // XCD-blocked tile order (launch: xcd_block; compact_rows is free on plain launches):
      // XCD x = blockIdx.x % 8 owns an a x b block of output tiles, a = compact_rows M tiles,
      // so its L2 fetches a rows of A panels and b columns of W panels from the MALL instead
      // of all of A (splitk 1, tile counts divisible as the host checked)
      const int a = compact_rows, b = (ntile >> 3) / a, gm = tiles_m / a;
      const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
      tm = (xcd % gm) * a + idx % a;
      tn = (xcd / gm) * b + idx / a;
      ks = 0;
    }
    glds_tile<C, LN, (POL & 1) ? kPolStream : 0, false, false, 0, false,
              ((POL & 2) ? kPolStream : 0) | ((POL & 4) ? kPolWT : 0)>(
        smem, A, lda, W, ldw, Cp, ldc, bias, R, ldr, part, M, M, N, K, act, alpha, ks, kslice, tm, tn, ln_colsum,
        (LN || ep.ext_stats) ? ln_mode : 0, ln_eps, ep);
    return;
  }
  // device-side row range (MoE expert): the host launched ONE tile row (tiles_m == 1) — no
  // idle blocks holding CUs — and each block walks the range's M tiles of its column panel
  const int r0 = rows[0], Mr = compact_rows ? min(rows[1] - r0, compact_rows) : rows[1] - r0;
  A += (size_t)r0 * lda;
  if (!compact_rows) Cp += (size_t)r0 * ldc;
  if (R) R += (size_t)r0 * ldr;
  if (part) part += (size_t)r0 * N;
  for (int t = 0; t * C::BM < Mr; ++t) {
    if (t) raw_barrier();  // every wave is done reading the staging buffers of the previous tile
    glds_tile<C, 0, 0, false, false, 0, false, 0, 2>(smem, A, lda, W, ldw, Cp, ldc, bias, R, ldr, part, Mr, M, N, K, act,
                                                     alpha, ks, kslice, t, tn, ln_colsum, 0, ln_eps, ep);
  }
}

// XCD-blocked tile order for a plain launch: the M-tile count a of each XCD's a x b block of
// output tiles (a x b = tiles / 8, the 8 blocks tiling the grid) that minimises the operand
// panels one XCD's L2 fetches, a * (A panel bytes) + b * (W panel bytes), when that beats the
// default order (32 consecutive tiles, M fastest) by 10 %; 0 = default order. Off unless
// DLS_XCD_BLOCK=1: on GPT-2's out-proj / fc2 (16 x 16 tiles, 8 x 4 blocks per XCD: 26 % fewer
// panel bytes per L2) the step measured 0.3 % slower (profiles/r4_ab/xcd_grouping.txt).
inline int xcd_block(int tiles_m, int tiles_n, size_t a_bytes, size_t w_bytes) {
  static const bool on = [] {
    const char* e = std::getenv("DLS_XCD_BLOCK");
    return e && *e == '1';
  }();
  const int ntile = tiles_m * tiles_n;
  if (!on || ntile % 8 || ntile < 64) return 0;
  const int per = ntile / 8;
  const size_t cur = (size_t)std::min(per, tiles_m) * a_bytes + (size_t)((per + tiles_m - 1) / tiles_m) * w_bytes;
  size_t best = cur;
  int best_a = 0;
  for (int a = 1; a <= per; ++a) {
    if (per % a || tiles_m % a) continue;
    const int b = per / a;
    if (tiles_n % b || (tiles_m / a) * (tiles_n / b) != 8) continue;
    const size_t c = (size_t)a * a_bytes + (size_t)b * w_bytes;
    if (c < best) {
      best = c;
      best_a = a;
    }
  }
  return best * 10 < cur * 9 ? best_a : 0;
}

// resident blocks of a persistent launch: CUs x blocks per CU (occupancy query, cached)
template <class C, int LN>
int persistent_grid() {
  static int g = 0;
  if (!g) {
    int dev = 0, cus = 256, per = 1;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, gemm_glds_kernel<C, LN, 2>, C::T, 0);
    g = cus * (per > 0 ? per : 1);
  }
  return g;
}

template <class C>
bool launch(const GemmArgs& a, int splitk, float* ws, hipStream_t s, const float* ln_colsum, int ln_mode,
            float ln_eps, const int* rows, bool persist) {
  // in-launch combine only while the last arriver's serial read of the other slices stays small
  // (cdna_hip_programming.md: ~1 us per 16 KB; Llama-3-8B's 256x128 split-4 tiles would read
  // 384 KB in one block, far slower than the reduce kernel)
  // (DLS_FIXUP_MAX_KB: the largest slab read, in KiB, for which the combine stays in-launch)
  static const int fixup_max = [] {
    const char* e = std::getenv("DLS_FIXUP_MAX_KB");
    return (e && *e ? std::atoi(e) : 64) * 1024;
  }();
  const bool fixup = splitk > 1 && !rows && (splitk - 1) * C::BM * C::BN * 4 <= fixup_max;
  // policy stores are buffer stores with 32-bit byte offsets from the output's base: outputs
  // (or split-K slabs) of 2 GB and more keep the default stores
  int spol = a.stream_pol & 7;
  if ((size_t)a.M * a.ldc * 2 >= (1ull << 31) || (size_t)a.M * a.N * 4 * splitk >= (1ull << 31)) spol &= 1;
  // ep.w_stream carries the store policy to the split-K reduce kernels (grouped launches alone
  // read it as the weight policy)
  const Epi ep{a.rope, a.stats_out, a.ext_stats, fixup ? a.tile_sem : nullptr, nullptr, nullptr, spol & 4};
  const int crows = rows ? a.compact_rows
                         : (!persist && splitk == 1 ? xcd_block((a.M + C::BM - 1) / C::BM, (a.N + C::BN - 1) / C::BN,
                                                                (size_t)C::BM * a.K * 2, (size_t)C::BN * a.K * 2)
                                                    : 0);
  static_assert(2 * C::BM * sizeof(float) <= C::LDS_UNITS * 16, "LN stats must fit the staging LDS");
  const int tiles_m = rows ? 1 : (a.M + C::BM - 1) / C::BM, tiles_n = (a.N + C::BN - 1) / C::BN;
  const int kslice = a.K / splitk;
  const int total = tiles_m * tiles_n * splitk;
  dim3 grid(total), block(C::T);
#define DLS_K(LN_, RG_, ...)                                                                                      \
  hipLaunchKernelGGL((gemm_glds_kernel<C, LN_, RG_, ##__VA_ARGS__>), grid, block, 0, s, (const bf16*)a.A, a.lda, (const bf16*)a.W, \
                     a.ldw, (bf16*)a.C, a.ldc, (const bf16*)a.bias, (const bf16*)a.R, a.ldr, ws, a.M, a.N, a.K, a.act, \
                     a.alpha, tiles_m, tiles_n, splitk, kslice, ln_colsum, ln_mode, ln_eps, rows, crows, ep)
  const bool ln_in = ln_mode != 0 && !a.ext_stats;
  if (rows) DLS_K(0, 1);
  else if (persist) {
    if (ln_in) {
      if constexpr (C::BM * C::BN <= 256 * 128 && C::KG == 1) {
        grid = dim3(std::min(total, persistent_grid<C, 1>()));
        DLS_K(1, 2);
      }
    } else {
      grid = dim3(std::min(total, persistent_grid<C, 0>()));
      DLS_K(0, 2);
    }
  } else if (ln_in) {
    if constexpr (C::BM * C::BN <= 256 * 128 && C::KG == 1) DLS_K(1, 0);  // 256x256: no registers left for it
  } else {
    const int pol = spol;  // an own kernel per policy
    switch (pol) {
      case 1: DLS_K(0, 0, 1); break;
      case 2: DLS_K(0, 0, 2); break;
      case 3: DLS_K(0, 0, 3); break;
      case 4: DLS_K(0, 0, 4); break;
      case 5: DLS_K(0, 0, 5); break;
      default: DLS_K(0, 0);
    }
  }
#undef DLS_K
  if (splitk > 1 && !ep.tile_sem) return glds_reduce(a, splitk, ws, s, ln_colsum, ln_mode, ln_eps, rows, ep);
  return false;
}

using C0 = Cfg<256, 128, 4, 2, 3>;  // 8 waves, 64x64 per wave: large GEMMs
using C1 = Cfg<128, 128, 2, 2, 3>;  // 4 waves, 64x64 per wave
using C2 = Cfg<128, 64, 2, 2, 4>;   // 4 waves, 64x32 per wave
using C3 = Cfg<64, 64, 2, 2, 4>;    // 4 waves, 32x32 per wave
using C4 = Cfg<64, 128, 2, 2, 4>;
using C5 = Cfg<64, 64, 2, 2, 8>;    // deep pipeline: 7 K-tiles in flight (cold-weight latency)
using C6 = Cfg<128, 64, 2, 2, 6>;   // 5 in flight, 2x rows per block
using C7 = Cfg<128, 128, 2, 2, 4>;
using C8 = Cfg<256, 256, 2, 4, 2>;     // 8 waves, 128x64 per wave, 2 x 64 KiB stages: big square-ish GEMMs
using C9 = Cfg<256, 256, 2, 4, 2, 1>;  // same with s_setprio(1) around the MFMA cluster (T5)
using C10 = Cfg<256, 128, 4, 2, 3, 1>; // C0 with s_setprio
using C11 = Cfg<128, 128, 2, 2, 4, 1>; // C7 with s_setprio
// split rings: the cold weight stream one tile deeper than the L2-resident activations
using C12 = Cfg<256, 256, 2, 4, 2, 0, 1>;  // 2 x 32 KiB A + 3 x 32 KiB W = 160 KiB
using C13 = Cfg<256, 256, 2, 4, 2, 1, 1>;
using C14 = Cfg<256, 128, 4, 2, 3, 0, 1>;  // 3 x 32 KiB A + 4 x 16 KiB W = 160 KiB
using C15 = Cfg<128, 128, 2, 2, 3, 0, 1>;  // 3 x 16 KiB A + 4 x 16 KiB W
// two K groups (8 waves, intra-block split-K) for the skinny M = 512 GEMMs
using C16 = Cfg<64, 64, 2, 2, 3, 0, 0, 2>;   // 3 x 32 KiB stages
using C17 = Cfg<64, 64, 2, 2, 2, 0, 0, 2>;   // 2 x 32 KiB: two blocks per CU
using C18 = Cfg<128, 64, 2, 2, 2, 0, 0, 2>;  // 2 x 48 KiB
using C19 = Cfg<64, 128, 2, 2, 2, 0, 0, 2>;
using C20 = Cfg<64, 64, 2, 2, 2, 0, 0, 4>;   // four K groups: 16 waves, 2 x 64 KiB stages
using C21 = Cfg<64, 64, 1, 2, 2, 0, 0, 4>;   // four K groups of 2 waves (64x32 each)
// tiles sized so a 512-row GEMM covers the 256 CUs exactly once (per-CU L2->LDS bytes, not
// MFMA rate, bound these: 512x3072 -> 8x32 tiles of 64x96, 512x2304 -> 16x16 of 32x144,
// 512x768 -> 16x16 of 32x48)
using C22 = Cfg<64, 96, 2, 2, 4>;
using C23 = Cfg<32, 144, 2, 1, 4>;
using C24 = Cfg<32, 48, 2, 1, 4>;
using C25 = Cfg<64, 96, 2, 2, 3, 0, 0, 2>;
using C26 = Cfg<32, 144, 2, 1, 3, 0, 0, 2>;
using C27 = Cfg<32, 48, 2, 1, 4, 0, 0, 2>;
// 128x128 with two K groups: each stage's DMA covers 256 contiguous bytes of every weight row
// (two K-tiles back to back) — the HBM-streaming MoE expert GEMMs (128 routed rows, cold weights)
using C28 = Cfg<128, 128, 2, 2, 2, 0, 0, 2>;
// 192-row tiles: a top-2 expert of a 512-token batch gets ~128 +- 11 routed rows, so 128-row
// tiles need a second pass over the WHOLE weight panel for most experts; 192 rows take any
// such expert in one pass (its weights stream from HBM exactly once)
using C29 = Cfg<192, 128, 2, 2, 3>;
using C30 = Cfg<192, 128, 2, 2, 2, 0, 0, 2>;
using C31 = Cfg<192, 128, 2, 2, 2, 0, 1>;  // split rings: 2 x 24 KiB A + 3 x 16 KiB W
// deeper split rings for the HBM-streaming expert GEMMs: 3 x 24 KiB A + 4 x 16 KiB W = 136 KiB
// keeps 2 A and 3 W tiles in flight (C31: 1 and 2); C33 issues them from 8 waves (48 x 64 wave
// tiles). Measured (Mixtral-8x7B grouped launches): C33 441 / 206 us for gate-up / down vs C31
// 465 / 215; C32 (same rings, 4 waves) no faster than C31 — the wave count, not the ring
// depth, moved it. A 192 x 256 tile (half the routed-row bytes per weight byte) ran > 550 us.
// Role-split rings (half the waves DMA only W, 5-6 tiles deep; the other half only A, 2 deep;
// 8 or 16 waves) were slower still: 537-545 / 254-268 us — not bytes in flight but the number of
// DMA-issuing waves per stream bounds these launches.
using C32 = Cfg<192, 128, 2, 2, 3, 0, 1>;
using C33 = Cfg<192, 128, 4, 2, 3, 0, 1>;
// 256 x 256 with the half-tile ring main loop (mainloop_ring): LM heads and the large GEMMs
using C34 = Cfg<256, 256, 2, 4, 2, 0, 0, 1, 1>;
using C35 = Cfg<256, 256, 2, 4, 2, 1, 0, 1, 1>;
// 224-column tiles: a 512-row GEMM whose N is a multiple of 7 x 32 fills the 256 CUs in whole
// rounds (Llama-3-8B gate/up N = 28672 -> 2 x 128 = 256 tiles of 256 x 224; 256 x 256 leaves 32
// CUs idle), and the GPT-2 LM head (N = 50304) takes 450 tiles = 1.76 rounds instead of 394
// tiles of 256 x 256 whose second round is half empty. Split rings: 2 x 32 KiB A + 3 x 28 KiB W.
using C36 = Cfg<256, 224, 4, 2, 2, 0, 1>;  // wave 64 x 112 (plain epilogues)
using C37 = Cfg<256, 224, 8, 1, 2, 0, 1>;  // wave 32 x 224: SwiGLU gate/up pairs (multiples of 32)
// 128 x 96 / 128 x 64 tiles of 8 waves for the long-K projections (K = 4096: 512 x 6144 ->
// 4 x 64 = 256 tiles, 512 x 4096 -> 4 x 64 = 256 tiles of 128 x 64) without split-K partials
using C38 = Cfg<128, 96, 4, 2, 4>;             // wave 32 x 48, 4 x 28 KiB stages
using C39 = Cfg<128, 96, 2, 2, 2, 0, 0, 2>;    // two K groups of wave 64 x 48, 2 x 56 KiB stages
using C40 = Cfg<128, 64, 2, 2, 3, 0, 0, 2>;    // two K groups of wave 64 x 32, 3 x 48 KiB stages
// MoE experts (192 routed rows, cold weights): the W ring TWO tiles deeper than the A ring —
// 3 x 24 KiB A + 5 x 16 KiB W = 152 KiB, four weight tiles (64 KiB) in flight per CU (C33: 3)
using C41 = Cfg<192, 128, 4, 2, 3, 0, 2>;
// 256 x 144 tiles of 8 waves (wave 32 x 144): the TAIL of a wide GEMM whose first columns ran
// as one whole round of 256 x 256 tiles — the GPT-2 LM head's last 17,489 columns as 244 tiles
// (one round) instead of 138 more 256 x 256 tiles that leave 118 CUs idle (ops.linear_norm
// column split, ops/gemm_tuning.json "col_splits"). 3 x 50 KiB joint stages.
using C42 = Cfg<256, 144, 8, 1, 3>;
// 256 x 192 tiles, 8 waves as 4 x 2 (wave 64 x 96), split rings 2 x 32 KiB A + 3 x 24 KiB W:
// with split-K 4 a 512 x 6144 x 4096 projection (Llama-3 QKV) is 64 tiles x 4 slices = 256
// blocks whose per-CU operand bytes are half those of the one-slice 128 x 96 tiles
using C43 = Cfg<256, 192, 4, 2, 2, 0, 1>;
// MoE gate/up: 160 routed rows (an expert's whole row range at 512 tokens top-2 over 8 experts)
// x 256 weight columns, wave 80 x 64, split rings 2 x 20 KiB A + 3 x 32 KiB W: 80 B of operand
// intake per output instead of 102 for 192 x 128 (the gathered A rows are re-read per column tile)
using C44 = Cfg<160, 256, 2, 4, 2, 0, 1>;
// GPT-2's skinny N = 768 GEMMs: 32 x 48 tiles with FOUR K groups (8 waves issuing the LDS-DMA
// of each 256-deep super-step instead of 4): more DMA issuers per CU for the intake-bound K loop
using C45 = Cfg<32, 48, 2, 1, 3, 0, 0, 4>;
// Two workgroups per CU (the MoE expert launches expose per-workgroup latency
// with one 512-thread workgroup per CU): 4-wave 128 x 128 tiles in at most 80 KiB of LDS, so a
// second workgroup's DMA and MFMAs run while the first waits at its barrier — joint rings of 2
// stages (64 KiB), and split rings with the weight ring one deeper (2 x 16 KiB A + 3 x 16 KiB W)
using C46 = Cfg<128, 128, 2, 2, 2, 0, 0, 1, 0, 2>;
using C47 = Cfg<128, 128, 2, 2, 2, 0, 1, 1, 0, 2>;
// (measured and dropped: the same tile with 2 or 4 stages, with eight K groups, and fc1 as one
// round of 64 x 96 tiles with four K groups — profiles/r4_ab/gpt2_n768_cfg45.txt)
// (and the MoE experts' 192 x 128 tile with two K groups, 16 waves: Mixtral 28.7 / 42.6 ms
// with it on down / gate-up against 24.3 — profiles/r4_ab/moe_gateup_cfg44.txt)

// the Mixtral down tile's taller form (busiest expert per layer: 149-227 routed rows,
// profiles/r6_mixtral/rows_vs_time.txt): 192 -> 256 rows (config 14; the grouped kernel keeps
// 241 VGPRs, no scratch).
// gate/up (160 x 256): 224 x 256 (wave 112 x 64, split rings 2 x 28 KiB A + 3 x 32 KiB W),
// instantiated below — the grouped kernel spills 68 VGPRs with it (a 320 x 128 half-panel form
// spilled 132-172)
template <>
struct TallTile<C44> {
  using type = Cfg<224, 256, 2, 4, 2, 0, 1>;
};
template <>
struct TallTile<C33> {
  using type = C14;
};

template <class C>
void grouped(const GemmArgs& a, int n_groups, const int* offsets, const unsigned long long* w_ptrs,
             const unsigned long long* c_ptrs, hipStream_t s, const int* a_rows) {
  // expert weights (read once per step, far larger than the MALL) are DMA'd with the nt
  // policy: Mixtral-8x7B 27.05 vs 27.89 ms per step (DLS_EXPERT_NT=0 restores the default)
  static const int w_stream = [] {
    const char* e = std::getenv("DLS_EXPERT_NT");
    return e && e[0] == '0' ? 0 : 1;
  }();
  // (the nt path DMAs the A rows by buffer loads with 32-bit offsets: an A of 2 GB or more
  // takes the default path)
  // row-split pairs (kernel: RANGED == 3): DLS_EXPERT_PAIRS=0 one block walks every row tile,
  // 1 same-XCD partners, 2 (default) partners in the grid's second half, 3 in its first half
  // (read per launch — a captured step replays without it — so a test can switch modes)
  const char* pe = std::getenv("DLS_EXPERT_PAIRS");
  const int pairs = pe && *pe ? std::atoi(pe) : 2;
  const int pair = a.grouped_shared ? 0 : pairs;
  // DLS_EXPERT_XCD=1: XCD-affine block order (kernel: RANGED == 3)
  const char* xe = std::getenv("DLS_EXPERT_XCD");
  const bool xcd = xe && *xe == '1' && !a.grouped_shared && pair != 1;
  // DLS_EXPERT_TALL (default 1): an expert past the tile's rows but within its TallTile's takes
  // one taller pass (configs with a TallTile only): Mixtral-8x7B 24.18-24.25 -> 23.72-23.81 ms
  // (profiles/r6_ab/expert_tall_tile.txt)
  const char* te = std::getenv("DLS_EXPERT_TALL");
  const bool tall = !(te && *te == '0') && !a.grouped_shared;
  const Epi ep{a.rope, nullptr, nullptr, nullptr, w_ptrs, c_ptrs,
               (a.grouped_shared ? 8 : ((size_t)a.M * a.lda * 2 < (1ull << 31) ? w_stream : 0)) |
                   (pair == 1 ? 16 : pair == 2 ? 32 : pair == 3 ? 64 : 0) | (xcd ? 128 : 0) | (tall ? 256 : 0)};
  const int tiles_n = (a.N + C::BN - 1) / C::BN;
  const int blocks = pair == 1 ? (n_groups * tiles_n + 7) / 8 * 16 : pair >= 2 ? 2 * n_groups * tiles_n
                                                                               : n_groups * tiles_n;
  // (tiles_m carries the group count: the paired walk bounds its pair index by it)
  hipLaunchKernelGGL((gemm_glds_kernel<C, 0, 3>), dim3(blocks), dim3(C::T), 0, s, (const bf16*)a.A, a.lda,
                     nullptr, a.ldw, (bf16*)a.C, a.ldc, nullptr, nullptr, 0,
                     const_cast<float*>(reinterpret_cast<const float*>(a_rows)), a.M, a.N, a.K, a.act, a.alpha,
                     n_groups, tiles_n, 1, a.K, nullptr, 0, 1e-5f, offsets, a.compact_rows, ep);
}

// ---- Wave-private rings: a barrier-free K loop for the 32 x 48 tiles (kGemmPrivate ids) ----
//
// The K-grouped tiles above move every stage with the whole block: each K super-step all waves
// wait, pass one s_barrier and issue their share of the next stage together. Here each of the W
// waves owns a contiguous slice of K and an LDS ring of its own (S slots of one 64-deep K-tile:
// 80 rows x 128 B = 10 KiB, 4 DMA instructions for the A rows and 6 for the W rows), multiplies
// the WHOLE 32 x 48 tile over its slice (FM = 2, FN = 3: 24 accumulator registers) and meets the
// other waves only once, at the barrier of the finish. Ordering inside the loop is the wave's own:
//  * RAW: a wave reads only bytes its own DMA instructions wrote, behind its own counted vmcnt
//    wait (vmcnt retires in order). The barrier that rule asks for elsewhere is for OTHER readers
//    of the staged bytes; there are none.
//  * WAR: a slot is re-issued only behind an lgkmcnt(0) that follows the ds_reads of it (LDS
//    returns in order: every read of the slot has delivered), pinned by sched_barrier(0) on both
//    sides of the refill.
// Every wave executes the same instruction counts whatever its slice holds, and no wave leaves
// before the finish: the kernel's one barrier cannot be missed (the host refuses a K whose tiles
// do not divide by W, and the grid is exactly the tile count — no idle block, no early return).
// PrivTile is the family over its tile: PrivCfg<W, S> the 32 x 48 tiles of ids kGemmPrivate..,
// 64 x 96 and 64 x 80 the folded-norm tiles of ids kGemmPrivateWide.. (gemm_private_wide_kernel).
template <int BM_, int BN_, int W_, int S_>
struct PrivTile {
  static constexpr int W = W_, S = S_, BM = BM_, BN = BN_, BK = 64, CH = 8, FM = BM / 16, FN = BN / 16;
  static constexpr int T = 64 * W, PW = (BM + BN) / 8;  // DMA instructions per K-tile
  static constexpr int SLOT = (BM + BN) * CH;            // bf16x8 units of one K-tile image
  static constexpr int RING = S * SLOT, LDS_UNITS = W * RING;
  static constexpr int REG = FM * FN * 64;               // f32x4 records of a wave's fragments
  static_assert(BM % 16 == 0 && BN % 16 == 0, "whole 16 x 16 fragments");
  static_assert(S >= 1 && PW * (S - 1) <= 63, "vmcnt range");
  static_assert(LDS_UNITS * 16 <= 163840 && T <= 1024, "LDS budget, block size");
  static_assert(REG <= RING, "a wave's fragment region lies inside its own ring");
};
template <int W_, int S_>
using PrivCfg = PrivTile<32, 48, W_, S_>;

template <class P>
__device__ __forceinline__ void mainloop_private(bf16x8* ring, const bf16* __restrict__ A, int lda,
                                                 const bf16* __restrict__ W, int ldw, int M, int N, int m0, int n0,
                                                 int kbeg, int nk, int lane, f32x4 (&acc)[P::FM][P::FN]) {
  const bf16* src[P::PW];
#pragma unroll
  for (int j = 0; j < P::PW; ++j) {
    const int row = 8 * j + (lane >> 3);
    const int kofs = kbeg + ((lane & 7) ^ (row & 7)) * 8;
    src[j] = row < P::BM ? A + (size_t)min(m0 + row, M - 1) * lda + kofs
                         : W + (size_t)min(n0 + row - P::BM, N - 1) * ldw + kofs;
  }
  auto issue = [&](int kt, bf16x8* slot) {
#pragma unroll
    for (int j = 0; j < P::PW; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(src[j] + kt * P::BK),
                                       (__attribute__((address_space(3))) void*)(slot + j * 64), 16, 0, 0);
  };
#pragma unroll
  for (int s = 0; s < P::S; ++s)
    if (s < nk) issue(s, ring + s * P::SLOT);
  int sl = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tiles kt+1 .. kt+S-1 were issued after kt and may stay in flight (kt+S goes out below)
    wait_tiles<P::PW, P::S - 1>(min(P::S - 1, nk - 1 - kt));
    bf16x8* slot = ring + sl * P::SLOT;
    const bf16x8* sA = slot;
    const bf16x8* sB = slot + P::BM * P::CH;
    bf16x8 af[2][P::FM], bw[2][P::FN];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int j = 0; j < P::FN; ++j) {
        const int row = j * 16 + (lane & 15);
        bw[kk][j] = sB[row * P::CH + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int i = 0; i < P::FM; ++i) {
        const int row = i * 16 + (lane & 15);
        af[kk][i] = sA[row * P::CH + (chunk ^ (row & 7))];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every read of the slot has returned (WAR)
    __builtin_amdgcn_sched_barrier(0);
    if (kt + P::S < nk) issue(kt + P::S, slot);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < P::FM; ++i)
#pragma unroll
        for (int j = 0; j < P::FN; ++j) acc[i][j] = mfma16x16x32(bw[kk][j], af[kk][i], acc[i][j]);
    sl = sl + 1 == P::S ? 0 : sl + 1;
  }
}

// C = alpha * A @ W^T + bias (+ R), row statistics of the stored bf16 into stats_out: what GPT-2's
// out-proj and fc2 attach. The finish is the one-pass finish of the K-grouped tiles with W regions:
// each wave writes its six fp32 fragments into a region at the start of ITS OWN ring (its last
// vmcnt(0) retired every DMA into that ring and its MFMAs consumed every read of it: no barrier
// before the write), ONE barrier, and thread tid < 256 sums the W records of its 16-byte row
// segment in ascending wave order, finishes and stores it — the same expression, operand
// requests and store as glds_tile's one-pass finish.
template <class P, int SPOL>
__global__ __launch_bounds__(P::T, 1) void gemm_private_kernel(const bf16* __restrict__ A, int lda,
                                                               const bf16* __restrict__ W, int ldw,
                                                               bf16* __restrict__ Cp, int ldc,
                                                               const bf16* __restrict__ bias,
                                                               const bf16* __restrict__ R, int ldr,
                                                               float* __restrict__ stats_out, int M, int N, int K,
                                                               float alpha, int tiles_m) {
  static_assert(P::T >= P::BM * 8, "one 16-byte output segment per storing thread");
  __shared__ bf16x8 smem[P::LDS_UNITS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile % tiles_m) * P::BM, n0 = (tile / tiles_m) * P::BN;
  DLS_STAMP(0)
  const int nk = K / (P::BK * P::W);  // K-tiles of every wave's slice
  bf16x8* ring = smem + wave * P::RING;
  f32x4 acc[P::FM][P::FN];
#pragma unroll
  for (int i = 0; i < P::FM; ++i)
#pragma unroll
    for (int j = 0; j < P::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  mainloop_private<P>(ring, A, lda, W, ldw, M, N, m0, n0, wave * nk * P::BK, nk, lane, acc);
  DLS_STAMP(1)
  // the segment's operands, requested in one batch behind the wave's last vmcnt wait (range-checked
  // buffer loads: rows past M and, with the vector forms, columns past N read zeros)
  constexpr int BNC = P::BN / 8, BNP = 8;
  const bool own = tid < P::BM * BNP;  // (wave-uniform: four whole waves)
  const int rl = tid / BNP, cc = tid % BNP;
  const int row = m0 + rl, col = n0 + cc * 8;
  const bool pre_bvec = ((reinterpret_cast<uintptr_t>(bias) & 7) | (N & 3)) == 0;
  const bool v16 = ((reinterpret_cast<uintptr_t>(Cp) | ((uintptr_t)ldc * 2)) & 15) == 0 &&
                   (!R || ((reinterpret_cast<uintptr_t>(R) | ((uintptr_t)ldr * 2)) & 15) == 0);
  const bool pre_res = R != nullptr && N >= 8 && v16 && ((size_t)(M + P::BM) * ldr * 2 < (1ull << 31));
  // (a bias that is not 8-byte aligned, or N % 4 != 0, is read in place behind the barrier: a second
  // batched form's registers would be written on this path behind the pending loads of the other)
  u32x2 o_bv[2];  // pre_bvec: 4 bf16 each
  u32x4 o_r;
  if (own) {
    constexpr int kRaw = 0x00020000;  // raw buffer, 32-bit data
    if (bias && pre_bvec) {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(bias), 0, N * 2, kRaw);
#pragma unroll
      for (int h = 0; h < 2; ++h) o_bv[h] = __builtin_amdgcn_raw_buffer_load_b64(rs, col * 2 + h * 8, 0, 0);
    }
    if (pre_res) {
      const auto rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(R), 0, (int)(((size_t)(M - 1) * ldr + N) * 2), kRaw);
      o_r = __builtin_amdgcn_raw_buffer_load_b128(rs, (row * ldr + col) * 2, 0, 0);
    }
  }
  // fragment records: glds_tile's one-pass layout with one wave per region (NW = 1)
  f32x4* reg = reinterpret_cast<f32x4*>(ring);
#pragma unroll
  for (int i = 0; i < P::FM; ++i)
#pragma unroll
    for (int j = 0; j < P::FN; ++j) {
      const int cl = j * 16 + (lane >> 4) * 4;
      reg[(i * P::FN + j) * 64 + (lane & 48) + ((lane & 15) ^ (((cl >> 3) & 3) << 2))] = acc[i][j];
    }
  epi_barrier<true>();  // THE barrier: every wave's fragments are in LDS (operand requests stay in flight)
  DLS_STAMP(7)
  if (own) {
    // (chunks past BNC read chunk BNC - 1 again and store nothing)
    const int ccr = min(cc, BNC - 1), cl0 = ccr * 8;
    const int rec = ((rl / 16) * P::FN + cl0 / 16) * 64 + (cl0 & 8) * 4 + ((rl & 15) ^ ((ccr & 3) << 2));
    const f32x4* red = reinterpret_cast<const f32x4*>(smem);
    f32x4 part_lo[P::W], part_hi[P::W];
#pragma unroll
    for (int w = 0; w < P::W; ++w) {
      part_lo[w] = red[w * P::RING + rec];
      part_hi[w] = red[w * P::RING + rec + 16];
    }
    f32x4 lo = part_lo[0], hi = part_hi[0];
#pragma unroll
    for (int w = 1; w < P::W; ++w) {
      lo += part_lo[w];
      hi += part_hi[w];
    }
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bias) {
      if (pre_bvec) {
        uint32_t w[8];  // (a bf16 is the high half of its fp32)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          consume_from_here(o_bv[h]);
          const uint32_t p0 = o_bv[h][0], p1 = o_bv[h][1];
          w[4 * h + 0] = p0 << 16;
          w[4 * h + 1] = p0 & 0xffff0000u;
          w[4 * h + 2] = p1 << 16;
          w[4 * h + 3] = p1 & 0xffff0000u;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = col + e < N ? __uint_as_float(w[e]) : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < N) bv[e] = bf2f(bias[col + e]);
      }
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(alpha * (e < 4 ? lo[e & 3] : hi[e & 3]) + bv[e]);
    if (pre_res) consume_from_here(o_r);
    // the residual add, the store and the row statistics of what was stored (glds_tile: store_segment)
    float s1 = 0.f, s2 = 0.f;
    if (cc < BNC && row < M && col < N) {
      if (v16 && col + 8 <= N) {
        if (R) {
          const bf16x8 r8 = pre_res ? *reinterpret_cast<const bf16x8*>(&o_r)
                                    : *reinterpret_cast<const bf16x8*>(R + (size_t)row * ldr + col);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(o[e]) + bf2f(r8[e]));
        }
        store16_pol<SPOL>(Cp, ((size_t)row * ldc + col) * 2, *reinterpret_cast<const u32x4*>(&o));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = bf2f(o[e]);
          s1 += y;
          s2 += y * y;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (col + e >= N) continue;
          float x = bf2f(o[e]);
          if (R) x += bf2f(R[(size_t)row * ldr + col + e]);
          const bf16 ob = f2bf(x);
          Cp[(size_t)row * ldc + col + e] = ob;
          const float y = bf2f(ob);
          s1 += y;
          s2 += y * y;
        }
      }
    }
    if (stats_out) {
#pragma unroll
      for (int o_ = 1; o_ < BNP; o_ <<= 1) {
        s1 += __shfl_xor(s1, o_, 64);
        s2 += __shfl_xor(s2, o_, 64);
      }
      if (cc == 0 && row < M) {
        atomicAdd(stats_out + 2 * row, s1);
        atomicAdd(stats_out + 2 * row + 1, s2);
      }
    }
  }
  DLS_STAMP(3)
}

// Whether the wave-private family takes this launch: plain 32 x 48 tiles of the whole K, nothing
// attached but bias / residual / stats_out / alpha (the callers fall back to the table's previous
// config, or refuse a forced id).
inline bool private_takes(int waves, const GemmArgs& a, int splitk, bool folded_norm, bool ranged) {
  return waves > 0 && a.K > 0 && a.K % (64 * waves) == 0 && splitk <= 1 && !folded_norm && !ranged &&
         a.act == ACT_NONE && a.rope.cols == 0 && !a.ext_stats;
}

template <int W_, int S_>
void launch_private(const GemmArgs& a, hipStream_t s) {
  using P = PrivCfg<W_, S_>;
  const int tiles_m = (a.M + P::BM - 1) / P::BM, tiles_n = (a.N + P::BN - 1) / P::BN;
  dim3 grid(tiles_m * tiles_n), block(P::T);
#define DLS_PK(POL_)                                                                                               \
  hipLaunchKernelGGL((gemm_private_kernel<P, POL_>), grid, block, 0, s, (const bf16*)a.A, a.lda, (const bf16*)a.W, \
                     a.ldw, (bf16*)a.C, a.ldc, (const bf16*)a.bias, (const bf16*)a.R, a.ldr, a.stats_out, a.M, a.N, \
                     a.K, a.alpha, tiles_m)
  // (the output stores' cache policy, GemmArgs::stream_pol bits 1 and 2, as launch<C> maps them:
  // policy stores carry 32-bit byte offsets, outputs of 2 GB and more keep the default stores)
  switch ((size_t)a.M * a.ldc * 2 < (1ull << 31) ? a.stream_pol & 7 : 0) {
    case 2: case 3: DLS_PK(kPolStream); break;
    case 4: case 5: DLS_PK(kPolWT); break;
    default: DLS_PK(0);
  }
#undef DLS_PK
}

// ---- Wave-private rings, 64-row tiles with the folded-norm finish (kGemmPrivateWide ids) ----
//
// C = act(rstd * (A @ W'^T - mu * colsum(W')) + bias): what GPT-2's QKV and fc1 attach — a folded
// norm (either mode) whose row statistics come from ext_stats, bias, no activation or GeLU. The K
// loop is mainloop_private on a 64 x 96 or 64 x 80 tile (one tile per CU at 512 x 3072 and
// 512 x 2304: a whole round); the finish is the one above with more segments than threads: every
// wave writes its FM * FN fragments into a region at the start of its own ring, ONE barrier, and
// the threads walk the tile's 16-byte segments in T-wide passes, each summing the W records of
// its segment in ascending wave order and finishing it with finish_value. A pass maps 16
// consecutive threads to 4 consecutive chunks of 4 consecutive rows (the conflict-free read of
// glds_tile's record layout); BN = 80 leaves the last quad of chunks half empty. All operands of
// all passes are requested in one batch behind the wave's last vmcnt wait.
template <class P, int SPOL>
__global__ __launch_bounds__(P::T, 1) void gemm_private_wide_kernel(const bf16* __restrict__ A,
                                                                    const bf16* __restrict__ W, bf16* __restrict__ Cp,
                                                                    const bf16* __restrict__ bias,
                                                                    const float* __restrict__ ln_colsum,
                                                                    const float* __restrict__ ext_stats, int lda,
                                                                    int ldw, int ldc, int M, int N, int K, int tiles_m,
                                                                    int ln_mode, int act, float ln_eps) {
  constexpr int BNC = P::BN / 8, NQ = (BNC + 3) / 4;  // 16-byte chunks of a tile row, quads of them
  constexpr int SEGS = P::BM * NQ * 4, NPASS = SEGS / P::T;
  static_assert(SEGS % P::T == 0, "whole passes: no thread without a segment");
  __shared__ bf16x8 smem[P::LDS_UNITS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile % tiles_m) * P::BM, n0 = (tile / tiles_m) * P::BN;
  DLS_STAMP(0)
  const int nk = K / (P::BK * P::W);  // K-tiles of every wave's slice
  bf16x8* ring = smem + wave * P::RING;
  f32x4 acc[P::FM][P::FN];
#pragma unroll
  for (int i = 0; i < P::FM; ++i)
#pragma unroll
    for (int j = 0; j < P::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  mainloop_private<P>(ring, A, lda, W, ldw, M, N, m0, n0, wave * nk * P::BK, nk, lane, acc);
  DLS_STAMP(1)
  // pass p: segment q = tid + p T -> chunk 4 (q / 16 % NQ) + q % 4 of tile row 4 (q / 16 / NQ) + q / 4 % 4
  auto seg_row = [&](int p) { const int q = tid + p * P::T; return (q >> 4) / NQ * 4 + ((q >> 2) & 3); };
  auto seg_chunk = [&](int p) { const int q = tid + p * P::T; return (q >> 4) % NQ * 4 + (q & 3); };
  // (range-checked buffer loads: rows past M and, with the vector forms, columns past N read zeros;
  // a bias / colsum that is not aligned, or N % 4 != 0, is read in place behind the barrier)
  const bool pre_bvec = ((reinterpret_cast<uintptr_t>(bias) & 7) | (N & 3)) == 0;
  const bool pre_cvec = ((reinterpret_cast<uintptr_t>(ln_colsum) & 15) | (N & 3)) == 0;
  const bool v16 = ((reinterpret_cast<uintptr_t>(Cp) | ((uintptr_t)ldc * 2)) & 15) == 0;
  u32x2 o_st[NPASS];     // fp32 bits of the row's (sum, sum of squares)
  u32x2 o_bv[NPASS][2];  // pre_bvec: 4 bf16 each
  u32x4 o_cs[NPASS][2];  // pre_cvec: fp32 bits
  {
    constexpr int kRaw = 0x00020000;  // raw buffer, 32-bit data
    const auto rst = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ext_stats), 0, M * 8, kRaw);
#pragma unroll
    for (int p = 0; p < NPASS; ++p) o_st[p] = __builtin_amdgcn_raw_buffer_load_b64(rst, (m0 + seg_row(p)) * 8, 0, 0);
    if (bias && pre_bvec) {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(bias), 0, N * 2, kRaw);
#pragma unroll
      for (int p = 0; p < NPASS; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          o_bv[p][h] = __builtin_amdgcn_raw_buffer_load_b64(rs, (n0 + seg_chunk(p) * 8) * 2 + h * 8, 0, 0);
    }
    if (pre_cvec) {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ln_colsum), 0, N * 4, kRaw);
#pragma unroll
      for (int p = 0; p < NPASS; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          o_cs[p][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, (n0 + seg_chunk(p) * 8) * 4 + h * 16, 0, 0);
    }
  }
  // fragment records: glds_tile's one-pass layout with one wave per region (NW = 1)
  f32x4* reg = reinterpret_cast<f32x4*>(ring);
#pragma unroll
  for (int i = 0; i < P::FM; ++i)
#pragma unroll
    for (int j = 0; j < P::FN; ++j) {
      const int cl = j * 16 + (lane >> 4) * 4;
      reg[(i * P::FN + j) * 64 + (lane & 48) + ((lane & 15) ^ (((cl >> 3) & 3) << 2))] = acc[i][j];
    }
  epi_barrier<true>();  // THE barrier: every wave's fragments are in LDS (operand requests stay in flight)
  DLS_STAMP(7)
  // Three phases, so that the sums and the values are straight-line code: (1) every pass's W
  // records summed in ascending wave order; (2) every pass's operands decoded (the in-place reads
  // of an unaligned bias / colsum branch here); (3) every value; then (below) every store —
  // vmcnt counts stores too, so a store between two passes would turn the next pass's wait for
  // its (long landed) operands into a wait for that store's round trip.
  const f32x4* red = reinterpret_cast<const f32x4*>(smem);
  f32x4 lo[NPASS], hi[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int rl = seg_row(p);
    // (chunks past BNC read chunk BNC - 1 again and store nothing)
    const int ccr = min(seg_chunk(p), BNC - 1), cl0 = ccr * 8;
    const int rec = ((rl / 16) * P::FN + cl0 / 16) * 64 + (cl0 & 8) * 4 + ((rl & 15) ^ ((ccr & 3) << 2));
    f32x4 part_lo[P::W], part_hi[P::W];
#pragma unroll
    for (int w = 0; w < P::W; ++w) {
      part_lo[w] = red[w * P::RING + rec];
      part_hi[w] = red[w * P::RING + rec + 16];
    }
    lo[p] = part_lo[0], hi[p] = part_hi[0];
#pragma unroll
    for (int w = 1; w < P::W; ++w) {
      lo[p] += part_lo[w];
      hi[p] += part_hi[w];
    }
  }
  const float inv_k = 1.0f / (float)K;
  float rs[NPASS], mu[NPASS], bv[NPASS][8], csv[NPASS][8];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int col = n0 + seg_chunk(p) * 8;
    consume_from_here(o_st[p]);
    const float a = __uint_as_float(o_st[p][0]), q = __uint_as_float(o_st[p][1]);
    mu[p] = ln_mode == 1 ? a * inv_k : 0.f;
    rs[p] = rsqrtf(fmaxf(q * inv_k - mu[p] * mu[p], 0.f) + ln_eps);
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[p][e] = csv[p][e] = 0.f;
    if (bias) {
      if (pre_bvec) {
        uint32_t w[8];  // (a bf16 is the high half of its fp32)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          consume_from_here(o_bv[p][h]);
          const uint32_t p0 = o_bv[p][h][0], p1 = o_bv[p][h][1];
          w[4 * h + 0] = p0 << 16;
          w[4 * h + 1] = p0 & 0xffff0000u;
          w[4 * h + 2] = p1 << 16;
          w[4 * h + 3] = p1 & 0xffff0000u;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[p][e] = col + e < N ? __uint_as_float(w[e]) : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < N) bv[p][e] = bf2f(bias[col + e]);
      }
    }
    if (pre_cvec) {
#pragma unroll
      for (int h = 0; h < 2; ++h) consume_from_here(o_cs[p][h]);
#pragma unroll
      for (int e = 0; e < 8; ++e) csv[p][e] = col + e < N ? __uint_as_float(o_cs[p][e >> 2][e & 3]) : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (col + e < N) csv[p][e] = ln_colsum[col + e];
    }
  }
  bf16x8 seg[NPASS];
  auto finish = [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
    for (int p = 0; p < NPASS; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        seg[p][e] = f2bf(finish_value<ACT, true>(e < 4 ? lo[p][e & 3] : hi[p][e & 3], 1.f, rs[p], mu[p], csv[p][e],
                                                 bv[p][e]));
  };
  if (act == ACT_GELU_TANH) finish(std::integral_constant<int, ACT_GELU_TANH>{});
  else finish(std::integral_constant<int, ACT_NONE>{});
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int cc = seg_chunk(p), row = m0 + seg_row(p), col = n0 + cc * 8;
    if (cc < BNC && row < M && col < N) {
      if (v16 && col + 8 <= N) {
        store16_pol<SPOL>(Cp, ((size_t)row * ldc + col) * 2, *reinterpret_cast<const u32x4*>(&seg[p]));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < N) Cp[(size_t)row * ldc + col + e] = seg[p][e];
      }
    }
  }
  DLS_STAMP(3)
}

// Whether the 64-row wave-private family takes this launch: the whole K in one block with
// K % (64 W) == 0, a folded norm whose row statistics come from ext_stats, bias, no activation or
// GeLU — no RoPE, SwiGLU, split-K, row range, residual or stats_out (the callers fall back to the
// table's previous config, or refuse a forced id).
inline bool private_wide_takes(int waves, const GemmArgs& a, int splitk, int ln_mode, bool ranged) {
  return waves > 0 && a.K > 0 && a.K % (64 * waves) == 0 && splitk <= 1 && (ln_mode == 1 || ln_mode == 2) &&
         a.ext_stats && !ranged && (a.act == ACT_NONE || a.act == ACT_GELU_TANH) && a.rope.cols == 0 && !a.R &&
         !a.stats_out;
}

template <int BM_, int BN_, int W_, int S_>
void launch_private_wide(const GemmArgs& a, const float* ln_colsum, int ln_mode, float ln_eps, hipStream_t s) {
  using P = PrivTile<BM_, BN_, W_, S_>;
  const int tiles_m = (a.M + P::BM - 1) / P::BM, tiles_n = (a.N + P::BN - 1) / P::BN;
  dim3 grid(tiles_m * tiles_n), block(P::T);
#define DLS_PK(POL_)                                                                                              \
  hipLaunchKernelGGL((gemm_private_wide_kernel<P, POL_>), grid, block, 0, s, (const bf16*)a.A, (const bf16*)a.W, \
                     (bf16*)a.C, (const bf16*)a.bias, ln_colsum, a.ext_stats, a.lda, a.ldw, a.ldc, a.M, a.N, a.K, \
                     tiles_m, ln_mode, a.act, ln_eps)
  // (the output stores' cache policy as launch_private maps it)
  switch ((size_t)a.M * a.ldc * 2 < (1ull << 31) ? a.stream_pol & 7 : 0) {
    case 2: case 3: DLS_PK(kPolStream); break;
    case 4: case 5: DLS_PK(kPolWT); break;
    default: DLS_PK(0);
  }
#undef DLS_PK
}

}  // namespace

// external entry points of config ID (declared in gemm_glds_cfgs.h)
#define DLS_GLDS_DEFINE(ID)                                                                                     \
  bool glds_launch_cfg##ID(const GemmArgs& a, int splitk, float* ws, hipStream_t s, const float* ln_colsum,     \
                           int ln_mode, float ln_eps, const int* rows, bool persist) {                          \
    return launch<C##ID>(a, splitk, ws, s, ln_colsum, ln_mode, ln_eps, rows, persist);                          \
  }                                                                                                             \
  void glds_grouped_cfg##ID(const GemmArgs& a, int n_groups, const int* offsets, const unsigned long long* w_ptrs, \
                            const unsigned long long* c_ptrs, hipStream_t s, const int* a_rows) {               \
    grouped<C##ID>(a, n_groups, offsets, w_ptrs, c_ptrs, s, a_rows);                                            \
  }
