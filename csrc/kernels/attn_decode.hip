// KV cache and decode attention, bf16 caches: the bf16 instances of the decode-attention kernel of
// attn_decode_impl.h (read that header for the kernel), kv_append, decode_prologue and the public
// entry points of both cache formats.
#include <algorithm>

#include "common.h"
#include "kernels.h"

#include "attn_decode_impl.h"

namespace {

using dls_attn::swz;

// bf16 rows: a K fragment is one 16-byte LDS read, and the 16-bit transposed read hands a lane
// eight keys of ONE d, so o[ng][dn][i] <-> d = 16dn + 4g + i of column ng*16 + li
struct Bf16Cache {
  using Elem = bf16;
  static constexpr int SCALE_BYTES = 0;
  struct Operands {
    const bf16 *K, *V;
    template <class F>
    void each(F f) const { f(K, V); }
  };
  static Operands operands(const DecodeArgs& a) {
    return {static_cast<const bf16*>(a.k_cache), static_cast<const bf16*>(a.v_cache)};
  }

  template <class Cf>
  static __device__ __forceinline__ bf16x8 k_frag(const char* kb, int row, int ks, int g) {
    const int ch = 4 * ks + g;
    return *reinterpret_cast<const bf16x8*>(kb + row * Cf::RB + ((ch ^ swz(row, Cf::CH - 1)) << 4));
  }

  template <class Cf>
  static __device__ __forceinline__ void pv(const bf16x4& lo, const bf16x4& hi, int dn, int ks,
                                            const bf16x8 (&pf)[Cf::NG][2], f32x4 (&o)[Cf::NG][Cf::ND]) {
    const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
    for (int ng = 0; ng < Cf::NG; ++ng) o[ng][dn] = mfma16x16x32(vf, pf[ng][ks], o[ng][dn]);
  }
};

// rows pos[b] + t of the caches <- rows b*T + t of the step's K and V, 16 bytes per thread
__global__ __launch_bounds__(256) void kv_append_kernel(const bf16* __restrict__ k_new, int ldk,
                                                        const bf16* __restrict__ v_new, int ldv,
                                                        bf16* __restrict__ k_cache, bf16* __restrict__ v_cache,
                                                        const int* __restrict__ pos, int T, int C, int row_elems,
                                                        int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int chunks = row_elems / 8;
  const int row = idx / (2 * chunks), rem = idx % (2 * chunks);
  const int op = rem / chunks, ch = rem % chunks;
  const int b = row / T, t = row % T;
  const int dst = pos[b] + t;
  if (dst < 0 || dst >= C) return;  // past the capacity: dropped
  const bf16* src = (op ? v_new + (size_t)row * ldv : k_new + (size_t)row * ldk) + ch * 8;
  bf16* out = (op ? v_cache : k_cache) + ((size_t)b * C + dst) * row_elems + ch * 8;
  *reinterpret_cast<u32x4*>(out) = *reinterpret_cast<const u32x4*>(src);
}

// block = one new token (b, t): its token id and its rows of up to two position tables
__global__ __launch_bounds__(128) void decode_prologue_kernel(const int* __restrict__ pos,
                                                              const int* __restrict__ tokens,
                                                              int* __restrict__ tok_out, const char* __restrict__ tab0,
                                                              char* __restrict__ out0, int rb0,
                                                              const char* __restrict__ tab1, char* __restrict__ out1,
                                                              int rb1, int T, int C) {
  const int row = blockIdx.x, b = row / T, t = row % T;
  const int p = min(max(pos[b] + t, 0), C - 1);
  if (threadIdx.x == 0 && tokens) tok_out[row] = tokens[(size_t)b * C + p];
  if (tab0)
    for (int i = threadIdx.x * 16; i < rb0; i += 128 * 16)
      *reinterpret_cast<u32x4*>(out0 + (size_t)row * rb0 + i) =
          *reinterpret_cast<const u32x4*>(tab0 + (size_t)p * rb0 + i);
  if (tab1)
    for (int i = threadIdx.x * 16; i < rb1; i += 128 * 16)
      *reinterpret_cast<u32x4*>(out1 + (size_t)row * rb1 + i) =
          *reinterpret_cast<const u32x4*>(tab1 + (size_t)p * rb1 + i);
}

}  // namespace

bool attn_decode_supported(int T, int n_head, int n_kv_head, int D) {
  return T >= 1 && T <= 16 && n_kv_head >= 1 && n_head % n_kv_head == 0 && n_head / n_kv_head * T <= 64 &&
         (D == 64 || D == 128);
}

int attn_decode_chunk(int B, int C, int n_kv_head, int D) {
  const int kts = D == 64 ? 256 : 128;  // keys per stage: a chunk is a whole number of stages
  // as many chunks as fill 256 CUs in one round of workgroups (one is resident per CU: 128 KB of
  // LDS), never a few more than that
  const int want = std::max(1, 256 / (n_kv_head * B));
  const int kc = ((C + want - 1) / want + kts - 1) / kts * kts;
  return std::max(kc, kts);
}

void attn_decode_sizes(const DecodeArgs& a, size_t* part_floats, size_t* counters) {
  const int KC = dls_decode::chunk_of(a);
  const size_t maxc = (a.C + KC - 1) / KC;
  *counters = (size_t)a.B * a.n_kv_head;
  *part_floats = *counters * maxc * (dls_decode::chunk_bytes(a.D, dls_decode::col_groups(a)) / 4);
}

void launch_attn_decode(const DecodeArgs& a, hipStream_t s) {
  if (a.kv_fp8) return launch_attn_decode_fp8(a, s);  // attn_decode_fp8.hip
  dls_decode::launch_decode_any<Bf16Cache>(a, s);
}

void launch_kv_append(const void* k_new, int ldk, const void* v_new, int ldv, void* k_cache, void* v_cache,
                      float* k_scale, float* v_scale, const int* pos, int B, int T, int C, int row_elems,
                      int n_kv_head, hipStream_t s) {
  if (k_scale)  // e4m3 caches: attn_decode_fp8.hip
    return launch_kv_append_fp8(k_new, ldk, v_new, ldv, k_cache, v_cache, k_scale, v_scale, pos, B, T, C, n_kv_head,
                                row_elems / n_kv_head, s);
  const int total = B * T * 2 * (row_elems / 8);
  hipLaunchKernelGGL(kv_append_kernel, dim3((total + 255) / 256), dim3(256), 0, s, static_cast<const bf16*>(k_new),
                     ldk, static_cast<const bf16*>(v_new), ldv, static_cast<bf16*>(k_cache),
                     static_cast<bf16*>(v_cache), pos, T, C, row_elems, total);
}

void launch_decode_prologue(const int* pos, const int* tokens, int* tok_out, const void* tab0, void* out0,
                            int row_bytes0, const void* tab1, void* out1, int row_bytes1, int B, int T, int C,
                            hipStream_t s) {
  hipLaunchKernelGGL(decode_prologue_kernel, dim3(B * T), dim3(128), 0, s, pos, tokens, tok_out,
                     static_cast<const char*>(tab0), static_cast<char*>(out0), row_bytes0,
                     static_cast<const char*>(tab1), static_cast<char*>(out1), row_bytes1, T, C);
}
