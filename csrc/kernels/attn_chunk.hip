// Chunk attention over the KV cache: a prompt chunk of T queries per sequence (1 <= T <= 1024)
// against the sequence's cache rows, with the offset and the key count read from pos[b] in device
// memory, so one captured launch follows a growing and ragged batch.
//
// The work item is attention_impl.h's attn_item, unchanged: 16*NW queries of one (sequence, head)
// walking their causal key range in 64*KS-key stages. This file only adds the entry that turns
// pos[b] into the item's per-sequence bases and bounds:
//   S     = min(pos[b] + T, C)   keys of sequence b (the step's own rows are appended before)
//   Sq    = T, q_off = pos[b]    query row t sits at position pos[b] + t
//   ldk   = ldv = n_kv_head * D  over the [B][C][n_kv_head*D] cache, base b*C rows in
// The item clamps the DMA rows of its last tile to S - 1 and masks key >= S, so cache rows at or
// past pos[b] + T are never read; rows of a loaded tile that the causal mask hides enter the
// second MFMA with p = 0, as in attention.hip. The grid is (ceil(T / QB), n_head, B) whatever pos
// holds. No key split across workgroups, no tickets, no workspace.
//
// kv_dequantize_rows: rows 0 .. min(pos[b]+T, C)-1 of an e4m3 cache times their power-of-two
// scales into a bf16 workspace of the cache's shape (exact: three mantissa bits times a power of
// two is a bf16 value); the chunk kernel then runs on the workspace.
// kv_advance: pos[b] = min(pos[b] + T, max(limit[b], pos[b])).
#include "common.h"
#include "kernels.h"

#include "attention_impl.h"

namespace {

using dls_attn::AttnCfg;

template <int D, int NW, int ST, int KS>
__global__ __launch_bounds__(64 * NW * KS) void attn_chunk_kernel(const bf16* __restrict__ Q, int ldq,
                                                                   const bf16* __restrict__ Kc,
                                                                   const bf16* __restrict__ Vc, bf16* __restrict__ O,
                                                                   int ldo, const int* __restrict__ pos, int T, int C,
                                                                   int n_head, int n_kv_head, float scale_log2,
                                                                   int n_qtiles) {
  using Cfg = AttnCfg<D, NW, ST, KS>;
  __shared__ __attribute__((aligned(16))) char smem[Cfg::SMEM];
  const int h = blockIdx.y, b = blockIdx.z;
  const int qt = n_qtiles - 1 - blockIdx.x;  // heaviest query tiles first
  const int p = min(max(pos[b], 0), C);
  const int S = min(p + T, C);  // >= 1
  const int ld = n_kv_head * D;
  const size_t kv0 = (size_t)b * C * ld;
  // batch 0 of the item with this sequence's bases: its own b*S / b*Sq row offsets vanish
  dls_attn::attn_item<D, NW, ST, KS, false, false>(smem, qt, 0, 1, h, 0, Q + (size_t)b * T * ldq, ldq, Kc + kv0, ld,
                                                   Vc + kv0, ld, O + (size_t)b * T * ldo, ldo, S, n_head, n_kv_head,
                                                   scale_log2, 1, n_qtiles, T, p, 0, nullptr, nullptr, 0);
}

template <int D, int NW, int ST, int KS>
void launch_cfg(const ChunkAttnArgs& a, hipStream_t s) {
  const int nq = (a.T + 16 * NW - 1) / (16 * NW);
  dim3 grid(nq, a.n_head, a.B), block(64 * NW * KS);
  hipLaunchKernelGGL((attn_chunk_kernel<D, NW, ST, KS>), grid, block, 0, s, static_cast<const bf16*>(a.q), a.ldq,
                     static_cast<const bf16*>(a.k_cache), static_cast<const bf16*>(a.v_cache),
                     static_cast<bf16*>(a.o), a.ldo, a.pos, a.T, a.C, a.n_head, a.n_kv_head,
                     a.scale * 1.4426950408889634f, nq);
}

template <int D>
void launch_d(const ChunkAttnArgs& a, hipStream_t s) {
  // the (NW, ST, KS) configurations of attention.hip's default choice, under its variant numbers
  switch (attn_chunk_variant(a.B, a.T, a.n_head, a.variant)) {
    case 13: launch_cfg<D, 2, 2, (D == 64 ? 4 : 2)>(a, s); break;
    case 8: launch_cfg<D, 4, 2, 2>(a, s); break;
    default: launch_cfg<D, 4, 2, 1>(a, s); break;
  }
}

// 8 cache bytes per thread: one 16-byte store of bf16
__global__ __launch_bounds__(256) void kv_dequantize_rows_kernel(const uint8_t* __restrict__ cache,
                                                                 const float* __restrict__ scale,
                                                                 const int* __restrict__ pos, bf16* __restrict__ out,
                                                                 int T, int C, int E, int D, int n_kv_head) {
  const int b = blockIdx.y;
  const int per_row = E / 8;
  const int idx = blockIdx.x * 256 + threadIdx.x;  // < C * E / 8 < 2^31 (checked by the binding)
  const int r = idx / per_row, j = idx - r * per_row;
  const int S = min(min(max(pos[b], 0), C) + T, C);
  if (r >= S) return;
  const size_t e0 = ((size_t)b * C + r) * E + (size_t)j * 8;
  const u32x2 w = *reinterpret_cast<const u32x2*>(cache + e0);
  const float sc = scale[((size_t)b * n_kv_head + (j * 8) / D) * C + r];
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    v[4 * i + 0] = f2bf(lo[0] * sc);
    v[4 * i + 1] = f2bf(lo[1] * sc);
    v[4 * i + 2] = f2bf(hi[0] * sc);
    v[4 * i + 3] = f2bf(hi[1] * sc);
  }
  *reinterpret_cast<bf16x8*>(out + e0) = v;
}

__global__ __launch_bounds__(256) void kv_advance_kernel(int* __restrict__ pos, const int* __restrict__ limit, int B,
                                                         int T) {
  for (int b = threadIdx.x; b < B; b += 256) {
    const int p = pos[b];
    pos[b] = min(p + T, max(limit[b], p));
  }
}

}  // namespace

bool attn_chunk_supported(int T, int n_head, int n_kv_head, int D) {
  return T >= 1 && T <= 1024 && n_kv_head >= 1 && n_head >= n_kv_head && n_head % n_kv_head == 0 &&
         (D == 64 || D == 128);
}

int attn_chunk_variant(int B, int T, int n_head, int variant) {
  if (variant == 2 || variant == 8 || variant == 13) return variant;
  // attention.hip's default by block count: 64-query blocks with two K/V stages fill the chip
  // from ~320 blocks on; below that the causal row's dependent chain is the kernel time, so each
  // stage's keys are split over wave groups
  const long blocks = (long)((T + 63) / 64) * n_head * B;
  return blocks <= 128 ? 13 : blocks <= 320 ? 8 : 2;
}

void launch_attn_chunk(const ChunkAttnArgs& a, hipStream_t s) {
  if (a.D == 64) launch_d<64>(a, s);
  else launch_d<128>(a, s);
}

void launch_kv_dequantize_rows(const void* cache, const float* scale, const int* pos, void* out, int B, int T, int C,
                               int n_kv_head, int D, hipStream_t s) {
  const int E = n_kv_head * D;
  const long groups = (long)C * (E / 8);
  hipLaunchKernelGGL(kv_dequantize_rows_kernel, dim3((unsigned)((groups + 255) / 256), B), dim3(256), 0, s,
                     static_cast<const uint8_t*>(cache), scale, pos, static_cast<bf16*>(out), T, C, E, D, n_kv_head);
}

void launch_kv_advance(int* pos, const int* limit, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(kv_advance_kernel, dim3(1), dim3(256), 0, s, pos, limit, B, T);
}
