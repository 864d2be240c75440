// Skinny W8A16 GEMM (the dense GEMMs of a decode step of an fp8-weight plan):
//   out[M][N'] = act(alpha * scale[n] * sum_k x[m][k] * q[n][k] + bias[n]) + R
// for 1 <= M <= 16 token rows of bf16 x, q stored as OCP e4m3 bytes [N][ldw] (K contiguous) and one
// fp32 scale per output channel; fp32 accumulation, bf16 output. The arithmetic is gemm_w8.hip's
// (bytes converted to bf16 in registers — exact for all 254 finite codes — products on the bf16
// MFMA, the channel scale applied once, in the epilogue, as (alpha * scale[n]) * acc + bias[n]); the
// structure is gemm_skinny.hip's, laid out again for 1-byte weights: the launch is a weight stream,
// every weight byte is needed once, by one wave. Weights go global -> VGPR in 16-byte loads through
// a two-slot register ring in a straight-line body; no LDS in the K loop and no barrier.
//
// Work split. A workgroup owns one 16-column strip of the output — for SwiGLU one 16-gate + 16-up
// block pair of the interleaved weight (and of the scales, interleaved the same way), which is 16
// outputs too; the grid is ceil(N / 16) (SwiGLU: N / 32). K is split INSIDE the workgroup: its W
// waves (template parameter, 4 / 8 / 16) take contiguous runs of 128-wide slices, each holds a
// 16 x 16 fp32 fragment (two for SwiGLU), and the finish is one LDS exchange: waves 1.. park their
// fragments, one barrier, wave 0 adds them to its own IN ASCENDING WAVE ORDER, applies the epilogue
// in fp32 and stores. No atomics and no split-K across workgroups: the same launch twice is
// bit-identical, and because a column of the MFMA's B operand only reaches its own token's outputs,
// row r of an M = 16 launch equals the M = 1 launch of that row bit for bit (same W).
//
// Slice. 128 k wide: one 128-byte line per fp8 weight row. Weight rows are the MFMA's A operand
// (lane l16 = weight row), token rows its B operand (lane l16 = token), so a lane's four accumulator
// values are four CONSECUTIVE output columns of one token row. Lane group g = lane >> 4 takes
// k = 32g..32g+31 of the slice: bytes [32g, 32g + 32) of its weight row — two adjacent 16-byte
// loads, so a wave's load pair covers 16 whole lines, each requested once — and the matching 64
// bytes of its token row, four 16-byte loads that stay in L2. The 32 weight bytes feed FOUR MFMA
// steps: step h converts bytes 8h..8h+7 (cvt_e4m3x8: byte i -> element i) and uses k = 32g + 8h..+7
// on both operands. Lanes of missing token rows repeat row M - 1 (same address, no extra traffic;
// nothing they compute is stored), and the lanes of a ragged last strip repeat weight row N - 1 and
// store nothing at columns >= N.
//
// Conversion: cvt_e4m3x8 of common.h (v_cvt_pk_f32_fp8 + the fp32 -> bf16 pack). The packed
// fp8 -> bf16 scale-convert of gfx950 was not measured against it; this is the form gemm_w8.hip
// holds exact.
//
// Epilogue (wave 0, fp32): (alpha * scale[n]) * acc + bias[n]; an activation (none / gelu-tanh /
// silu / relu / SwiGLU); ONE rounding to bf16; + residual; rounding; store — 8 bytes where
// ldc % 4 == 0, the base is 8-byte aligned and the four columns are inside N, scalar stores otherwise.
// No folded norm (W * gain would break the per-row scale) and no RoPE (fp8 plans keep the natural
// q/k layout): both stay their own launches.
#include "common.h"
#include "kernels.h"

namespace {

typedef const __attribute__((address_space(1))) u32x4 global_u32x4;

constexpr int BK = 128;  // K slice: one 128-byte line per weight row
constexpr int LK = 32;   // k of a slice per lane group: 32 weight bytes, 64 bytes of x
constexpr int PF = 2;    // slices in a wave's register ring (see gemm_grouped_skinny.hip)

struct SK8Params {
  const bf16* A;
  int lda;
  const uint8_t* Wq;
  int ldw;
  const float* scale;
  bf16* C;
  int ldc;
  const bf16* bias;
  const bf16* R;
  int ldr;
  int M, N, K;
  int act;
  float alpha;
};

// FN: weight fragments per strip (1 plain, 2 SwiGLU: gate block + up block); W: waves (K split)
template <int FN, int W>
__global__ __launch_bounds__(64 * W) void gemm_skinny_w8_kernel(const SK8Params p) {
  __shared__ f32x4 red[(W - 1) * FN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // in an SGPR: the K loop's branches are scalar
  const int l16 = lane & 15, g = lane >> 4;
  const int strip = blockIdx.x;
  const int K = p.K, N = p.N, M = p.M;

  // this wave's run of slices; K % 32 == 0, so a lane group of the last slice is whole or past K
  const int nk = (K + BK - 1) / BK, per = (nk + W - 1) / W;
  const int s0 = wave * per, s1 = min(nk, s0 + per);

  // lane (l16, g): bytes [32g, 32g + 32) of the line of weight row l16 of every fragment. Loads
  // are unconditional at clamped addresses (rows past N repeat row N - 1, slices past the run
  // repeat its last slice, k past K repeats the row's last 32 bytes) and what must not count is
  // zeroed where it is consumed.
  const uint8_t* wp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = p.Wq + (size_t)min(strip * 16 * FN + j * 16 + l16, N - 1) * p.ldw;
  const bf16* xp = p.A + (size_t)min(l16, M - 1) * p.lda;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  f32x4 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s0 < s1) {  // wave-uniform
    u32x4 wr[PF][FN][2], xr[PF][4];
    auto load = [&](int kt, u32x4(&w)[FN][2], u32x4(&x)[4]) {
      const int ko = min(min(kt, s1 - 1) * BK + LK * g, K - LK);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        global_u32x4* q = (global_u32x4*)(wp[j] + ko);
        w[j][0] = q[0];
        w[j][1] = q[1];
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
    // Main loop, ring and scheduling barriers: the bf16 kernel's. PF whole slices inside the run
    // per trip; the run's last slice, the only one that can reach past K, is always left to the
    // tail. A slot's loads are issued right after its MFMAs, so the wait in front of the other
    // slot's MFMAs is a counted one and this slot's loads stay in flight across the trip.
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

  // lane: token row l16, columns 4g..4g+3 of the strip
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < FN; ++j) red[((wave - 1) * FN + j) * 64 + lane] = acc[j];
  }
  __syncthreads();
  if (wave != 0) return;

  // value e of fragment j belongs to weight row wrow(j) + e: its scale and its bias, requested
  // together at clamped rows before the wave sum (eight dependent round trips otherwise)
  float sc[FN][4], bs[FN][4];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int wrow = min(strip * 16 * FN + j * 16 + 4 * g + e, N - 1);
      sc[j][e] = p.scale[wrow];
      bs[j][e] = p.bias ? bf2f(p.bias[wrow]) : 0.f;
    }

  // ascending wave order; a few waves per trip: unrolled whole, the 2 x 15 fragments of the
  // SwiGLU W = 16 instance would all be loaded before the first add
#pragma unroll 3
  for (int w = 0; w < W - 1; ++w)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x4 t = red[(w * FN + j) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] += t[e];
    }

  const int row = l16;
  if (row >= M) return;
  const int col = strip * 16 + 4 * g;  // output column of v[0]
  const int n_out = FN == 2 ? N / 2 : N;
  if (col >= n_out) return;
  const int nv = min(4, n_out - col);

  float v[FN][4];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[j][e] = e < nv ? (p.alpha * sc[j][e]) * acc[j][e] + bs[j][e] : 0.f;
  float o[4];
  if constexpr (FN == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = silu(v[0][e]) * v[1][e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = apply_act(v[0][e], p.act);
  }
  bf16x4 ob;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bf16 t = f2bf(o[e]);
    if (p.R && e < nv) t = f2bf(bf2f(t) + bf2f(p.R[(size_t)row * p.ldr + col + e]));
    ob[e] = t;
  }
  const size_t idx = (size_t)row * p.ldc + col;
  if (nv == 4 && (p.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.C) & 7) == 0)) {
    *reinterpret_cast<bf16x4*>(p.C + idx) = ob;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) p.C[idx + e] = ob[e];
  }
}

template <int FN>
void launch_w(const SK8Params& p, int strips, int waves, hipStream_t s) {
  if (waves == 16) hipLaunchKernelGGL((gemm_skinny_w8_kernel<FN, 16>), dim3(strips), dim3(64 * 16), 0, s, p);
  else if (waves == 8) hipLaunchKernelGGL((gemm_skinny_w8_kernel<FN, 8>), dim3(strips), dim3(64 * 8), 0, s, p);
  else hipLaunchKernelGGL((gemm_skinny_w8_kernel<FN, 4>), dim3(strips), dim3(64 * 4), 0, s, p);
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

int gemm_skinny_w8_waves(int N, int K, int act) {
  // From the kernel table (profiles/skinny_w8/kernels.txt), not from a model. The first rule — the
  // bf16 kernel's, by slices per wave: 8, 16 for a vocabulary-sized N at K >= 4096 — picked the
  // slowest instance for both LM heads (Llama: 129 us against 101 with four waves; GPT-2: 19 against
  // 11) and the second best elsewhere. Four waves are the fastest or within 4 % of it at every shape
  // and M measured, SwiGLU included: a 128-wide slice keeps twice the k of the bf16 kernel's in
  // flight per wave, so fewer waves cover the latency. The exception kept: K >= 8192 on a plain
  // strip (Llama's down-projection, 112 slices), where eight waves gain 3 % at M <= 4.
  (void)N;
  if (act == kActSwiglu) return 4;
  return (K + BK - 1) / BK >= 64 ? 8 : 4;
}

bool gemm_skinny_w8_takes(const GemmSkinnyW8Args& a, const char** why) {
  const char* r = nullptr;
  const int n_out = a.act == kActSwiglu ? a.N / 2 : a.N;
  if (a.M < 1 || a.M > kSkinnyMaxRows) r = "1 <= M <= 16 rows";
  else if (a.N < 1 || a.K < 32 || a.K % 32 != 0) r = "N >= 1 and K a positive multiple of 32";
  else if (a.lda % 8 != 0 || a.lda < a.K) r = "lda % 8 == 0 and lda >= K";
  else if (a.ldw % 16 != 0 || a.ldw < a.K) r = "ldw % 16 == 0 (bytes) and ldw >= K";
  else if (a.scale == nullptr) r = "one fp32 scale per weight row";
  else if (a.act < 0 || a.act > kActSwiglu) r = "act in none / gelu / silu / relu / swiglu";
  else if (a.act == kActSwiglu && a.N % 32 != 0) r = "SwiGLU needs N % 32 == 0";
  else if (a.waves != 0 && a.waves != 4 && a.waves != 8 && a.waves != 16) r = "waves in {4, 8, 16}";
  else if (a.ldc < n_out || (a.R != nullptr && a.ldr < n_out)) r = "ldc / ldr below the output width";
  if (why) *why = r;
  return r == nullptr;
}

bool launch_gemm_skinny_w8(const GemmSkinnyW8Args& a, hipStream_t s) {
  if (!gemm_skinny_w8_takes(a, nullptr) || !aligned16(a.A) || !aligned16(a.Wq)) return false;
  SK8Params p{};
  p.A = (const bf16*)a.A;
  p.lda = a.lda;
  p.Wq = (const uint8_t*)a.Wq;
  p.ldw = a.ldw;
  p.scale = a.scale;
  p.C = (bf16*)a.C;
  p.ldc = a.ldc;
  p.bias = (const bf16*)a.bias;
  p.R = (const bf16*)a.R;
  p.ldr = a.ldr;
  p.M = a.M;
  p.N = a.N;
  p.K = a.K;
  p.act = a.act;
  p.alpha = a.alpha;
  const int waves = a.waves ? a.waves : gemm_skinny_w8_waves(a.N, a.K, a.act);
  if (a.act == kActSwiglu) launch_w<2>(p, a.N / 32, waves, s);
  else launch_w<1>(p, (a.N + 15) / 16, waves, s);
  return true;
}
