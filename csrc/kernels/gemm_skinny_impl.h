// The e4m3 skinny GEMMs on MFMA: what gemm_skinny_w8.hip (dense) and gemm_grouped_skinny_w8.hip (MoE
// experts) share — the lane geometry and the K split, the K loop, the finish and the launch
// ladder, written once. Each file keeps its kernel: its params, its grid and row addressing, its
// epilogue, its dispatch rules. The bf16 kernels (gemm_skinny.hip, gemm_grouped_skinny.hip) are the
// same design on K loops of their own, for 2-byte weights and 64-wide slices.
//
// out = epi(x W^T) for AT MOST 16 token rows per pass. A decode step has M = B*T <= 16 token rows,
// so the launch is a weight stream: each weight byte is needed once, by one wave, and the
// arithmetic is free. This is the "GEMV / M <= 16 decode weights" form: weights go global -> VGPR
// in 16-byte loads through a two-slot register ring in a straight-line unrolled body; no LDS in
// the K loop and no barrier.
//
// Work split. A workgroup owns one column strip of the output: 16 columns — for SwiGLU one 16-gate +
// 16-up block pair of the interleaved weight, which is 16 outputs too — or, grouped only, 32 plain
// columns (two fragments sharing one token fragment: per lane two weight requests for every token
// request, where the 16-column form has one for two). K is split INSIDE the workgroup: its W waves
// take contiguous runs of slices, each holds a 16 x 16 fp32 fragment per weight fragment, and the
// finish is one LDS exchange: waves 1.. park their fragments, one barrier, wave 0 adds them to its
// own IN ASCENDING WAVE ORDER, applies the epilogue in fp32, rounds once to bf16 and stores. No
// atomics and no split-K across workgroups: the same launch twice is bit-identical.
//
// Operand layout. Operands are swapped as in gemm_w8_grouped.hip and attn_decode_impl.h: the weight
// rows are the MFMA's A operand (lane l16 = weight row), the <= 16 token rows its B operand
// (lane l16 = token), so a lane's four accumulator values are four CONSECUTIVE output columns of
// one token row — one 8-byte store — and a gate/up pair is two fragments of the same lane. A column
// of the B operand only reaches its own token's outputs, so row r of a 16-row launch equals the
// 1-row launch of that row bit for bit (same W), and whatever a clamped lane reads never reaches a
// stored element.
//
// Slice and k map. A slice is BK = 128 k wide: one 128-byte line per weight row. Lane group
// g = lane >> 4 takes k = 32g..32g+31 of it: bytes [32g, 32g + 32) of its weight row — two adjacent
// 16-byte loads, so a wave's load pair covers 16 whole lines, each requested exactly once — and
// the matching 64 bytes of its token row, four 16-byte loads. The 32 weight bytes feed FOUR MFMA
// steps: step h converts bytes 8h..8h+7 (cvt_e4m3x8: byte i -> element i, exact for all finite
// codes) and uses k = 32g + 8h..+7 on both operands; a sum over k does not care which k a lane
// holds as long as both operands agree. The token rows are a few KB that every strip of the launch
// re-reads, so they sit in L2, and lanes of missing token rows repeat the last row (same address,
// no extra traffic).
//
// Loads are unconditional at clamped addresses — weight rows past N repeat row N - 1, slices past
// the wave's run repeat its last slice (in flight or cached), k past K repeats the row's last 32
// bytes — and what must not count is zeroed where it is consumed: a select behind the load would
// make the wave wait at once.
//
// Ring. PF = 2 slices, as the bf16 kernels measured it (gemm_grouped_skinny.hip): 64 to 132 VGPRs,
// three to seven waves per SIMD, and it is the waves of several workgroups per CU, each with its
// slot's loads in flight, that keep the bytes coming while one of them is in its prologue or its
// finish.
//
// What the compiler emits for the waits (-O3, gfx950, read from the ISA of all eighteen instances;
// resource remarks in profiles/skinny_skeleton/): the ring stays in place, no instance uses scratch,
// every load and store is global_* (none flat). A slot holds 2 FN weight + 4 token loads, and BOTH
// waits of a trip are counted: in front of a slot's MFMAs the wave waits in steps down to
// vmcnt(4 + 2 FN) — vmcnt(14), (12), (8) with two fragments, vmcnt(10), (6) with one — which leaves
// the other slot's whole refill in flight, across trips too. No vmcnt(0) inside the loop (the bf16
// grouped kernel's first wait per trip is one); the tail waits vmcnt(4 + 2 FN) once more, then
// drains. No inline assembly was needed for it.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace dls_skinny {

// as in gemm_w8_grouped.hip: addresses that come from a device array need the global address
// space spelled out, or the loads and stores are FLAT and count against LDS waits too
typedef const __attribute__((address_space(1))) u32x4 global_u32x4;
typedef const __attribute__((address_space(1))) float global_f32;
typedef __attribute__((address_space(1))) bf16 global_bf16;
typedef __attribute__((address_space(1))) bf16x4 global_bf16x4;

constexpr int BK = 128;   // K slice: one 128-byte line per weight row
constexpr int LK = 32;    // k of a slice per lane group: 32 weight bytes, 64 bytes of x
constexpr int STEPS = 4;  // MFMA steps per slice, one 16-byte token load each
constexpr int PF = 2;     // slices in a wave's register ring

// lane (l16, g) of wave `wave`
struct Lanes {
  int lane, wave, l16, g;
};

__device__ __forceinline__ Lanes lanes() {
  Lanes q;
  q.lane = threadIdx.x & 63;
  q.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // in an SGPR: the K loop's branches are scalar
  q.l16 = q.lane & 15;
  q.g = q.lane >> 4;
  return q;
}

// a wave's run of slices [s0, s1) of the W-way K split. K % 32 == 0, so a lane group of the last
// slice is whole or past K.
template <int W>
__device__ __forceinline__ void run_of(int wave, int K, int& s0, int& s1) {
  const int nk = (K + BK - 1) / BK, per = (nk + W - 1) / W;
  s0 = wave * per;
  s1 = min(nk, s0 + per);
}

// lane (l16, g): bytes [32g, 32g + 32) of the line of weight row l16 of every fragment of the strip;
// rows past N (a ragged last strip) repeat row N - 1
template <int FN>
__device__ __forceinline__ void weight_rows(const uint8_t* Wq, size_t ldw, int strip, int l16, int N,
                                            const uint8_t* (&wp)[FN]) {
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = Wq + (size_t)min(strip * 16 * FN + j * 16 + l16, N - 1) * ldw;
}

// One wave's run of slices [s0, s1), s0 < s1: acc[j] += W_j x^T over the run (always inlined: the
// ring and the fragments are registers of the kernel).
template <int FN, bool NT>
__device__ __forceinline__ void run_k(const uint8_t* const (&wp)[FN], const bf16* xp, int g, int s0, int s1, int K,
                                      f32x4 (&acc)[FN]) {
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 wr[PF][FN][2], xr[PF][STEPS];
  auto load = [&](int kt, u32x4(&w)[FN][2], u32x4(&x)[STEPS]) {
    const int ko = min(min(kt, s1 - 1) * BK + LK * g, K - LK);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      global_u32x4* q = (global_u32x4*)(wp[j] + ko);
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
    for (int h = 0; h < STEPS; ++h) x[h] = q[h];
  };
  auto mma = [&](const u32x4(&w)[FN][2], const u32x4(&x)[STEPS]) {
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&x[h]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[j] = mfma16x16x32(cvt_e4m3x8(w[j][h >> 1][2 * (h & 1)], w[j][h >> 1][2 * (h & 1) + 1]), xf, acc[j]);
    }
  };
  // Main loop: PF whole slices inside the run per trip (the run's last slice, the only one that
  // can reach past K, is always left to the tail). Slice kt's MFMAs read ring slot kt % PF, then
  // the slot is refilled with slice kt + PF: a slot's loads are issued right after its MFMAs, so
  // the wait in front of the other slot's MFMAs is a counted one and leaves them in flight. The
  // scheduling barriers keep that order in the code and the ring in place (left alone, the
  // scheduler sank a trip's loads behind all its MFMAs and renamed the ring into 232 VGPRs).
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
  // on BOTH operands (a zero e4m3 byte converts to +0, and a NaN of x past K must not meet it)
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    const int kt = kt0 + s;
    const bool in = kt < s1 && kt * BK + LK * g < K;
    u32x4 w[FN][2], x[STEPS];
#pragma unroll
    for (int h = 0; h < STEPS; ++h) x[h] = in ? xr[s][h] : zero4;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < FN; ++j) w[j][h] = in ? wr[s][j][h] : zero4;
    mma(w, x);
  }
}

// The finish, around the kernel's one barrier: waves 1.. park their fragments in red
// [(W - 1) * FN * 64] ...
template <int FN>
__device__ __forceinline__ void park(f32x4* red, int wave, int lane, const f32x4 (&acc)[FN]) {
#pragma unroll
  for (int j = 0; j < FN; ++j) red[((wave - 1) * FN + j) * 64 + lane] = acc[j];
}

// ... and wave 0 adds them to its own in ascending wave order. A few waves per trip: unrolled
// whole, the 2 x 15 fragments of the SwiGLU W = 16 instance would all be loaded before the first
// add.
template <int FN, int W>
__device__ __forceinline__ void sum_waves(const f32x4* red, int lane, f32x4 (&acc)[FN]) {
#pragma unroll 3
  for (int w = 0; w < W - 1; ++w)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x4 t = red[(w * FN + j) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] += t[e];
    }
}

// Four rounded values of columns idx .. idx + 3 of C, the first nv of them inside the output: 8
// bytes where ldc % 4 == 0, the base is 8-byte aligned and all four are inside, scalar stores
// otherwise.
__device__ __forceinline__ void store4(global_bf16* C, size_t idx, int ldc, const bf16x4& ob, int nv) {
  if (nv == 4 && (ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 7) == 0)) {
    *reinterpret_cast<global_bf16x4*>(C + idx) = ob;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) C[idx + e] = ob[e];
  }
}

// Host side. The launch ladder: f is called with the compile-time constant of a run-time choice.
template <class Fn>
void by_bool(bool b, Fn&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// by_waves<16, 8, 4>(waves, f): f(integral_constant<int, W>) for the W that equals waves, else the last
template <int W0, int... Ws, class Fn>
void by_waves(int waves, Fn&& f) {
  if constexpr (sizeof...(Ws) == 0) f(std::integral_constant<int, W0>{});
  else if (waves == W0) f(std::integral_constant<int, W0>{});
  else by_waves<Ws...>(waves, f);
}

}  // namespace dls_skinny
