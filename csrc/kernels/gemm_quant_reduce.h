// gemm_quant_reduce.h: the split-K reduce kernel of the dense quantised GEMMs (gemm_w8.hip,
// gemm_w8a8.hip, gemm_w4a8.hip), written once. A format F names its kernel-argument struct
// (F::Params; read here: part, C, bias, R, ldc, ldr, M, N, act, alpha, pol and the scales the
// format has) and which factors scale the accumulator: kRowScale (xscale[m]), kColScale (scale[n]).
#pragma once
#include "common.h"

namespace {

// The accumulator's factor, associated as each format's main epilogue has it:
//   W8A16 (alpha * scale[n]) * acc      W8A8 (alpha * xscale[m]) * scale[n] * acc      W4A8 (alpha * xscale[m]) * acc
// A factor the format lacks is never computed: its variable stays 0 and scaled() does not read it.
template <class F>
__device__ __forceinline__ float row_factor(const typename F::Params& p, int row) {
  return p.alpha * p.xscale[row];
}
template <class F>
__device__ __forceinline__ float col_factor(const typename F::Params& p, int col) {
  if constexpr (F::kRowScale) return p.scale[col];
  else return p.alpha * p.scale[col];
}
template <class F>
__device__ __forceinline__ float scaled(float xs, float cs, float acc) {
  if constexpr (F::kRowScale && F::kColScale) return xs * cs * acc;
  else if constexpr (F::kRowScale) return xs * acc;
  else return cs * acc;
}

// out = epilogue(sum over the split slabs, slab 0 first). VEC output columns per thread
// (4 needs N % 4 == 0, NO % 4 == 0, ldc % 4 == 0, C 8-byte aligned; 1 takes anything).
template <class F, int VEC>
__global__ __launch_bounds__(256) void gemm_quant_reduce_kernel(const typename F::Params p, int splitk) {
  const bool sw = p.act == ACT_SWIGLU;
  const int M = p.M, N = p.N, NO = sw ? N / 2 : N;
  const int per_row = (NO + VEC - 1) / VEC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * per_row) return;
  const int row = (int)(idx / per_row), oc = (int)(idx % per_row) * VEC;
  const size_t slab = (size_t)M * N;
  float xs = 0.f;
  if constexpr (F::kRowScale) xs = row_factor<F>(p, row);
  float o[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int c = oc + e;
    // SwiGLU: output column c pairs weight rows 32b + j (gate) and 32b + 16 + j (up), c = 16b + j
    const int col = sw ? (c / 16) * 32 + (c % 16) : c;
    const float* P = p.part + (size_t)row * N + col;
    float a = 0.f, u = 0.f;
    for (int s = 0; s < splitk; ++s) {
      a += P[s * slab];
      if (sw) u += P[s * slab + 16];
    }
    float cs = 0.f, cu = 0.f;
    if constexpr (F::kColScale) cs = col_factor<F>(p, col);
    float v = scaled<F>(xs, cs, a) + (p.bias ? bf2f(p.bias[col]) : 0.f);
    if (sw) {
      if constexpr (F::kColScale) cu = col_factor<F>(p, col + 16);
      v = silu(v) * (scaled<F>(xs, cu, u) + (p.bias ? bf2f(p.bias[col + 16]) : 0.f));
    } else {
      v = apply_act(v, p.act);
    }
    if (p.R) v += bf2f(p.R[(size_t)row * p.ldr + c]);
    o[e] = v;
  }
  if constexpr (VEC == 4) {
    bf16x4 ob;
#pragma unroll
    for (int e = 0; e < 4; ++e) ob[e] = f2bf(o[e]);
    store_bf16x4(p.C, (size_t)row * p.ldc + oc, ob, p.pol);
  } else {
    p.C[(size_t)row * p.ldc + oc] = f2bf(o[0]);
  }
}

// p as the main kernel was launched with; splitk > 1
template <class F>
void launch_quant_reduce(const typename F::Params& p, int splitk, hipStream_t s) {
  const int NO = p.act == ACT_SWIGLU ? p.N / 2 : p.N;
  const bool vec = p.N % 4 == 0 && NO % 4 == 0 && p.ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(p.C) & 7) == 0;
  const long n = (long)p.M * (vec ? NO / 4 : NO);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (vec) hipLaunchKernelGGL((gemm_quant_reduce_kernel<F, 4>), grid, dim3(256), 0, s, p, splitk);
  else hipLaunchKernelGGL((gemm_quant_reduce_kernel<F, 1>), grid, dim3(256), 0, s, p, splitk);
}

}  // namespace
