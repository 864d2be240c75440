// Skinny W8A16 GEMM (the dense GEMMs of a decode step of an fp8-weight plan):
//   out[M][N'] = act(alpha * scale[n] * sum_k x[m][k] * q[n][k] + bias[n]) + R
// for 1 <= M <= 16 token rows of bf16 x, q stored as OCP e4m3 bytes [N][ldw] (K contiguous) and one
// fp32 scale per output channel; fp32 accumulation, bf16 output. The geometry, the K loop and the
// finish are gemm_skinny_impl.h's (the layout is explained there); W = 4 / 8 / 16 waves,
// default-policy weight loads. The arithmetic is gemm_w8.hip's: bytes converted to
// bf16 in registers — exact for all 254 finite codes — products on the bf16 MFMA, the channel scale
// applied once, in the epilogue.
//
// Conversion: cvt_e4m3x8 of common.h (v_cvt_pk_f32_fp8 + the fp32 -> bf16 pack). The packed
// fp8 -> bf16 scale-convert of gfx950 was not measured against it; this is the form gemm_w8.hip
// holds exact.
//
// Epilogue (wave 0, fp32): (alpha * scale[n]) * acc + bias[n]; an activation (none / gelu-tanh /
// silu / relu / SwiGLU, scales interleaved like the weight rows); ONE rounding to bf16; + residual;
// rounding; store. No folded norm (W * gain would break the per-row scale) and no RoPE (fp8 plans
// keep the natural q/k layout): both stay their own launches.
#include "gemm_skinny_impl.h"

namespace {

using namespace dls_skinny;

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

// One workgroup per strip, grid ceil(N / 16) (SwiGLU: N / 32). Lanes of missing token rows repeat
// row M - 1; the lanes of a ragged last strip repeat weight row N - 1 and store nothing at columns
// >= N. FN: weight fragments per strip (1 plain, 2 SwiGLU: gate block + up block); W: waves (K split)
template <int FN, int W>
__global__ __launch_bounds__(64 * W) void gemm_skinny_w8_kernel(const SK8Params p) {
  __shared__ f32x4 red[(W - 1) * FN * 64];
  const auto [lane, wave, l16, g] = lanes();
  const int strip = blockIdx.x;
  const int K = p.K, N = p.N, M = p.M;
  int s0, s1;
  run_of<W>(wave, K, s0, s1);

  const uint8_t* wp[FN];
  weight_rows(p.Wq, p.ldw, strip, l16, N, wp);
  const bf16* xp = p.A + (size_t)min(l16, M - 1) * p.lda;

  f32x4 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s0 < s1) run_k<FN, false>(wp, xp, g, s0, s1, K, acc);  // wave-uniform

  // lane: token row l16, columns 4g..4g+3 of the strip
  if (wave > 0) park(red, wave, lane, acc);
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
  sum_waves<FN, W>(red, lane, acc);

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
  store4((global_bf16*)p.C, (size_t)row * p.ldc + col, p.ldc, ob, nv);
}

template <int FN>
void launch(const SK8Params& p, int strips, int waves, hipStream_t s) {
  by_waves<16, 8, 4>(waves, [&](auto w) {
    hipLaunchKernelGGL((gemm_skinny_w8_kernel<FN, w()>), dim3(strips), dim3(64 * w()), 0, s, p);
  });
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
  if (a.act == kActSwiglu) launch<2>(p, a.N / 32, waves, s);
  else launch<1>(p, (a.N + 15) / 16, waves, s);
  return true;
}
