// Dense skinny GEMM (the dense GEMMs of a decode step): out[M][N'] = epi(alpha * x[M][K] * W[N][K]^T)
// for bf16 with 1 <= M <= 16 token rows. The dense sibling of gemm_grouped_skinny.hip and the same
// "GEMV / M <= 16 decode weights" form: the launch is a weight stream, every weight byte is needed
// once, by one wave, and the arithmetic is free. Weights go global -> VGPR in 16-byte loads through
// a two-slot register ring in a straight-line body; no LDS in the K loop and no barrier.
//
// Work split. A workgroup owns one 16-column strip of the output — for SwiGLU one 16-gate + 16-up
// block pair of the interleaved weight, which is 16 outputs too; the grid is ceil(N / 16) (SwiGLU:
// N / 32). K is split INSIDE the workgroup: its W waves (template parameter, 4 / 8 / 16) take
// contiguous runs of 64-wide slices, each holds a 16 x 16 fp32 fragment (two for SwiGLU), and the
// finish is one LDS exchange: waves 1.. park their fragments, one barrier, wave 0 adds them to its
// own IN ASCENDING WAVE ORDER, applies the epilogue in fp32 and stores. No atomics and no split-K
// across workgroups: the same launch twice is bit-identical, and because a column of the MFMA's B
// operand only reaches its own token's outputs, row r of an M = 16 launch equals the M = 1 launch
// of that row bit for bit (same W).
//
// Operand layout: as in gemm_grouped_skinny.hip. Weight rows are the MFMA's A operand (lane
// l16 = weight row), token rows its B operand (lane l16 = token), so a lane's four accumulator
// values are four CONSECUTIVE output columns of one token row. A slice is 64 wide and lane group
// g = lane >> 4 takes k = 16g..16g+15 of it — two adjacent 16-byte loads, 32 contiguous bytes —
// feeding MFMA step h with k = 16g + 8h..+7 on both operands; a wave's load pair covers 16 whole
// 128-byte lines of the weight, each requested once. Lanes of missing token rows repeat row M - 1
// (same address, no extra traffic; nothing they compute is stored), and the lanes of a ragged last
// strip repeat weight row N - 1 and store nothing at columns >= N.
//
// Folded norm. With ln_mode 1 (LayerNorm) / 2 (RMSNorm) x holds the RAW rows and the kernel takes
// the row statistics itself: every (token, k) of x is loaded by exactly one lane of the workgroup,
// which adds its values' sum and sum of squares in fp32 (what is past the wave's run or past K
// counts as zero); the four lane groups are added in the order 0, 1, 2, 3, the waves through the
// same LDS exchange in ascending order. Deterministic, and no producer has to emit statistics.
//
// Epilogue (wave 0, fp32): alpha; folded norm rstd * (acc - mean * colsum[n]) (RMSNorm: rstd * acc);
// bias; RoPE on pair-interleaved columns < cols (a lane's four columns are two whole pairs) or an
// activation (none / gelu-tanh / silu / relu / SwiGLU); ONE rounding to bf16; + residual; rounding;
// store — 8 bytes where ldc % 4 == 0, the base is 8-byte aligned and the four columns are inside
// N, scalar stores otherwise.
#include "common.h"
#include "kernels.h"

namespace {

typedef const __attribute__((address_space(1))) u32x4 global_u32x4;

constexpr int BK = 64;  // K slice: one 128-byte line per weight row
constexpr int PF = 2;   // slices in a wave's register ring (see gemm_grouped_skinny.hip)

struct SKParams {
  const bf16* A;
  int lda;
  const bf16* Wt;
  int ldw;
  bf16* C;
  int ldc;
  const bf16* bias;
  const bf16* R;
  int ldr;
  int M, N, K;
  int act;
  float alpha;
  RopeArgs rope;
  const float* colsum;
  int ln_mode;
  float ln_eps;
};

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// FN: weight fragments per strip (1 plain, 2 SwiGLU: gate block + up block); W: waves (K split);
// NT: streaming weight loads; LN: in-kernel row statistics for a folded norm
template <int FN, int W, bool NT, bool LN>
__global__ __launch_bounds__(64 * W) void gemm_skinny_kernel(const SKParams p) {
  __shared__ f32x4 red[(W - 1) * FN * 64];
  __shared__ float st_red[LN ? W * 32 : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // in an SGPR: the K loop's branches are scalar
  const int l16 = lane & 15, g = lane >> 4;
  const int strip = blockIdx.x;
  const int K = p.K, N = p.N, M = p.M;

  // this wave's run of slices; K % 32 == 0, so the last slice is whole or its lane groups 2, 3
  // are past K
  const int nk = (K + BK - 1) / BK, per = (nk + W - 1) / W;
  const int s0 = wave * per, s1 = min(nk, s0 + per);

  // lane (l16, g): bytes [32g, 32g + 32) of the line of weight row l16 of every fragment. Loads
  // are unconditional at clamped addresses (rows past N repeat row N - 1, slices past the run
  // repeat its last slice, k past K repeats the row's last 32 bytes) and what must not count is
  // zeroed where it is consumed.
  const bf16* wp[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) wp[j] = p.Wt + (size_t)min(strip * 16 * FN + j * 16 + l16, N - 1) * p.ldw;
  const bf16* xp = p.A + (size_t)min(l16, M - 1) * p.lda;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  f32x4 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float xs = 0.f, xq = 0.f;  // this lane's share of its token's sum and sum of squares

  if (s0 < s1) {  // wave-uniform
    u32x4 wr[PF][FN][2], xr[PF][2];
    auto load = [&](int kt, u32x4(&w)[FN][2], u32x4(&x)[2]) {
      const int ko = min(min(kt, s1 - 1) * BK + 16 * g, K - 16);
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
        if constexpr (LN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float a = bf_lo(x[h][e]), b = bf_hi(x[h][e]);
            xs += a;
            xq = fmaf(a, a, xq);
            xs += b;
            xq = fmaf(b, b, xq);
          }
        }
      }
    };
    // Main loop, ring and scheduling barriers: exactly the grouped kernel's (its comment explains
    // the pinning). PF whole slices inside the run per trip; the run's last slice, the only one
    // that can reach past K, is always left to the tail.
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

  // lane: token row l16, columns 4g..4g+3 of the strip
  if constexpr (LN) {
    // lane groups in the order 0, 1, 2, 3: every lane of the wave ends with its token's wave total
    const float a0 = __shfl(xs, l16, 64), a1 = __shfl(xs, l16 + 16, 64), a2 = __shfl(xs, l16 + 32, 64),
                a3 = __shfl(xs, l16 + 48, 64);
    const float q0 = __shfl(xq, l16, 64), q1 = __shfl(xq, l16 + 16, 64), q2 = __shfl(xq, l16 + 32, 64),
                q3 = __shfl(xq, l16 + 48, 64);
    xs = ((a0 + a1) + a2) + a3;
    xq = ((q0 + q1) + q2) + q3;
    if (wave > 0 && g == 0) {
      st_red[wave * 32 + 2 * l16] = xs;
      st_red[wave * 32 + 2 * l16 + 1] = xq;
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < FN; ++j) red[((wave - 1) * FN + j) * 64 + lane] = acc[j];
  }
  __syncthreads();
  if (wave != 0) return;

  // ascending wave order; a few waves per trip: unrolled whole, the 2 x 15 fragments of the
  // SwiGLU W = 16 instance are all loaded before the first add and spill
#pragma unroll 3
  for (int w = 0; w < W - 1; ++w)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x4 t = red[(w * FN + j) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] += t[e];
    }
  float mu = 0.f, rs = 1.f;
  if constexpr (LN) {
    for (int w = 1; w < W; ++w) {
      xs += st_red[w * 32 + 2 * l16];
      xq += st_red[w * 32 + 2 * l16 + 1];
    }
    const float inv_k = 1.0f / (float)K;
    mu = p.ln_mode == 1 ? xs * inv_k : 0.f;
    rs = rsqrtf(fmaxf(xq * inv_k - mu * mu, 0.f) + p.ln_eps);
  }

  const int row = l16;
  if (row >= M) return;
  const int col = strip * 16 + 4 * g;  // output column of v[0]
  const int n_out = FN == 2 ? N / 2 : N;
  if (col >= n_out) return;
  const int nv = min(4, n_out - col);

  // value e of fragment j belongs to weight row wrow(j) + e
  float v[FN][4];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int wrow = strip * 16 * FN + j * 16 + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = p.alpha * acc[j][e];
      if (e < nv) {
        if constexpr (LN) t = rs * (t - mu * p.colsum[wrow + e]);
        if (p.bias) t += bf2f(p.bias[wrow + e]);
      }
      v[j][e] = t;
    }
  }
  float o[4];
  if constexpr (FN == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = silu(v[0][e]) * v[1][e];
  } else {
    if (p.rope.cols > 0) rope_pairs<4>(v[0], row, col, p.rope);
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

template <int FN, int W, bool NT>
void launch_ln(const SKParams& p, int strips, hipStream_t s) {
  if (p.ln_mode != 0)
    hipLaunchKernelGGL((gemm_skinny_kernel<FN, W, NT, true>), dim3(strips), dim3(64 * W), 0, s, p);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<FN, W, NT, false>), dim3(strips), dim3(64 * W), 0, s, p);
}

template <int FN, int W>
void launch_nt(const SKParams& p, int strips, bool nt, hipStream_t s) {
  if (nt) launch_ln<FN, W, true>(p, strips, s);
  else launch_ln<FN, W, false>(p, strips, s);
}

template <int FN>
void launch_w(const SKParams& p, int strips, int waves, bool nt, hipStream_t s) {
  if (waves == 16) launch_nt<FN, 16>(p, strips, nt, s);
  else if (waves == 8) launch_nt<FN, 8>(p, strips, nt, s);
  else launch_nt<FN, 4>(p, strips, nt, s);
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

int gemm_skinny_waves(int N, int K, int act) {
  // From the kernel table (profiles/skinny_gemm/kernels.txt, waves_rule.txt), not from a model: the
  // first rule — the smallest W with strips * W >= 2048 and two slices per wave — picked the slowest
  // instance for GPT-2's fc2 (W 16) and the second best for most shapes. Eight waves are the fastest
  // or within 5 % of it at every plain shape measured, K = 768 (1.5 slices per wave) included;
  // SwiGLU's two fragments per wave are the fastest with four; a vocabulary-sized N at K >= 2048
  // (8016 strips: several workgroups per CU either way) gains another 3 % with sixteen.
  const int strips = act == kActSwiglu ? N / 32 : (N + 15) / 16;
  const int nk = (K + 63) / 64;
  if (act == kActSwiglu) return 4;
  if (strips >= 4096 && nk >= 32) return 16;
  return 8;
}

bool gemm_skinny_takes(const GemmSkinnyArgs& a, const char** why) {
  const char* r = nullptr;
  if (a.M < 1 || a.M > kSkinnyMaxRows) r = "1 <= M <= 16 rows";
  else if (a.N < 1 || a.K < 32 || a.K % 32 != 0) r = "N >= 1 and K a positive multiple of 32";
  else if (a.lda % 8 != 0 || a.ldw % 8 != 0 || a.lda < a.K || a.ldw < a.K) r = "lda % 8 == 0 and ldw % 8 == 0";
  else if (a.act < 0 || a.act > kActSwiglu) r = "act in none / gelu / silu / relu / swiglu";
  else if (a.act == kActSwiglu && a.N % 32 != 0) r = "SwiGLU needs N % 32 == 0";
  else if (a.rope.cols != 0 && (a.act != 0 || a.rope.cols % 4 != 0 || a.rope.cols < 0 || a.rope.cols > a.N ||
                                a.rope.D < 4 || a.rope.D % 4 != 0 || a.rope.cols % a.rope.D != 0 || a.rope.S < 1))
    r = "RoPE needs no activation, cols % 4 == 0, cols % D == 0, D % 4 == 0";
  else if (a.ln_mode < 0 || a.ln_mode > 2 || (a.ln_mode != 0 && a.ln_colsum == nullptr)) r = "norm mode 1 / 2 with colsum";
  else if (a.waves != 0 && a.waves != 4 && a.waves != 8 && a.waves != 16) r = "waves in {4, 8, 16}";
  else if (a.ldc < (a.act == kActSwiglu ? a.N / 2 : a.N) || (a.R != nullptr && a.ldr < (a.act == kActSwiglu ? a.N / 2 : a.N)))
    r = "ldc / ldr below the output width";
  if (why) *why = r;
  return r == nullptr;
}

bool launch_gemm_skinny(const GemmSkinnyArgs& a, hipStream_t s) {
  if (!gemm_skinny_takes(a, nullptr) || !aligned16(a.A) || !aligned16(a.W)) return false;
  SKParams p{};
  p.A = (const bf16*)a.A;
  p.lda = a.lda;
  p.Wt = (const bf16*)a.W;
  p.ldw = a.ldw;
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
  p.rope = a.rope;
  p.colsum = a.ln_colsum;
  p.ln_mode = a.ln_mode;
  p.ln_eps = a.ln_eps;
  const int waves = a.waves ? a.waves : gemm_skinny_waves(a.N, a.K, a.act);
  if (a.act == kActSwiglu) launch_w<2>(p, a.N / 32, waves, a.stream != 0, s);
  else launch_w<1>(p, (a.N + 15) / 16, waves, a.stream != 0, s);
  return true;
}
