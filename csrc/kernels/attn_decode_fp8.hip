// KV cache and decode attention with e4m3 caches: the quantising kv_append and the e4m3 instances
// of the decode-attention kernel of attn_decode_impl.h.
//
// Format: K and V bytes uint8 [B][C][n_kv_head*D] (OCP e4m3), scales fp32 [B][n_kv_head][C], one
// power-of-two scale per (position, KV head) by the rule of models/params.py quantize_fp8. An e4m3
// value times a power of two is a bf16 value, so what the kernel multiplies is exactly the
// dequantised bf16 row.
//
// attn_decode on e4m3: the grid, the chunk rule (attn_decode_chunk), the ticketed order-independent
// merge, the partial format and the workspace sizes are the shared kernel's. What the format does:
//  * A stage holds the same KTS keys as the bf16 instances', in half the bytes (16 KB per operand),
//    plus the stage's K and V scales (KTS fp32 each), which a wave fetches for its own 64 keys with
//    two 4-byte LDS-DMA instructions. The ring keeps two buffers (68 KB): a ring of four with three
//    stages in flight was measured and is slower (52.7 us against 49.3 us at Llama-3-8B, B = 8,
//    T = 1, P = 8192), so bytes in flight are not what limits this kernel.
//  * K: a lane reads the 8 bytes of its fragment (ds_read_b64), converts them to bf16 in registers
//    (v_cvt_scalef32_pk_bf16_fp8 with scale 1: two bytes to two bf16 per instruction, exact — the
//    selector tests hold it to the bit; v_cvt_pk_f32_fp8 plus a round to bf16 is twice the
//    instructions and measured 2 % slower) and runs the bf16 MFMA.
//  * V^T: a fragment is eight keys of one d per lane. The bytes are read with the 16-BIT transposed
//    read the bf16 kernel uses (ds_read_b64_tr_b16), each 16-bit element being the byte pair
//    (d = 2c, 2c+1) of one key: a lane receives column pair c = li of four keys per read. One
//    v_perm_b32 per word separates the even-d bytes from the odd-d bytes, and the two halves become
//    the A operands of TWO MFMAs: accumulator X = 2*dp + par holds, in row r of the MFMA,
//    d = 32*dp + 2*r + par. Rows of O^T are only relabelled — lane (g, li) ends up with the eight
//    consecutive d = 32*dp + 8*g .. +7 of its column, one 16-byte store. This uses only the lane
//    layout the bf16 kernel already relies on; the 8-bit transposed read (ds_read_b64_tr_b8), whose
//    layout benchmarks/ds_read_tr8_probe.hip prints, would save the v_perm but not a read.
//  * Scales are applied in the swapped-operand form, not while converting: in S^T = K Q^T a key is a
//    row of S^T, so the K scale multiplies the fp32 score of its key (NG*16 multiplies per tile,
//    against D per tile when converting), and in O^T += V^T P^T the V scale multiplies p of its key
//    before p is rounded to bf16. Both are exact (powers of two) and both use the SAME sixteen keys
//    per lane (16n + 4g + i), so each tile reads its scales as eight 16-byte LDS reads.
//  * Scales of keys that are not valid never reach arithmetic: the scale DMA clamps its index to the
//    chunk's last valid key exactly as the K/V rows are clamped, and a wave tile without a valid
//    key fetches nothing and is not computed.
//
// kv_append_fp8: 16 lanes per (row, KV head, operand), 8 elements per lane (D <= 128); the amax is
// reduced across those lanes in registers, then scale, bytes and one scale store. Byte for byte
// quantize_fp8 of the head row (up to the sign of a zero), the scale bit for bit.
#include "common.h"
#include "kernels.h"

#include "attn_decode_impl.h"
#include "attn_fp8_frag.h"

namespace {

using dls_fp8::Fp8Cache;  // the format's fragments, shared with attn_chunk_fp8.hip

// scale exponent e of quantize_fp8: amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9 (quant_rows.hip)
__device__ __forceinline__ int scale_exp(float amax) {
  int ex;
  const float m = frexpf(amax, &ex);
  return m <= 0.875f ? ex - 9 : ex - 8;
}

// 16 lanes = one (row, KV head, operand); lane l16 holds elements 8*l16 .. +7 of the head's D
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const bf16* __restrict__ k_new, int ldk,
                                                            const bf16* __restrict__ v_new, int ldv,
                                                            uint8_t* __restrict__ k_cache,
                                                            uint8_t* __restrict__ v_cache,
                                                            float* __restrict__ k_scale, float* __restrict__ v_scale,
                                                            const int* __restrict__ pos, int T, int C, int n_kv_head,
                                                            int D, int groups) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int l16 = idx & 15;
  const int grp = min(idx >> 4, groups - 1);  // a group past the end repeats the last one and stores nothing
  const bool live = (idx >> 4) < groups;
  const int op = grp % 2, h = grp / 2 % n_kv_head, row = grp / (2 * n_kv_head);
  const int b = row / T, t = row % T;
  const bool has = l16 * 8 < D;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (has) {
    const bf16* src = (op ? v_new + (size_t)row * ldv : k_new + (size_t)row * ldk) + h * D + l16 * 8;
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(src);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(x[i]);
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = group16_max(amax);
  const int dst = pos[b] + t;
  if (!live || dst < 0 || dst >= C) return;  // past the capacity: neither bytes nor scale
  const int e = amax > 0.f ? scale_exp(amax) : 0;
  if (l16 == 0) (op ? v_scale : k_scale)[((size_t)b * n_kv_head + h) * C + dst] = ldexpf(1.0f, e);
  if (!has) return;
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = fminf(fmaxf(ldexpf(v[i], -e), -448.f), 448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
  uint8_t* out = (op ? v_cache : k_cache) + ((size_t)b * C + dst) * ((size_t)n_kv_head * D) + h * D + l16 * 8;
  *reinterpret_cast<u32x2*>(out) = u32x2{(uint32_t)lo, (uint32_t)hi};
}

}  // namespace

void launch_attn_decode_fp8(const DecodeArgs& a, hipStream_t s) { dls_decode::launch_decode_any<Fp8Cache>(a, s); }

void launch_kv_append_fp8(const void* k_new, int ldk, const void* v_new, int ldv, void* k_cache, void* v_cache,
                          float* k_scale, float* v_scale, const int* pos, int B, int T, int C, int n_kv_head, int D,
                          hipStream_t s) {
  const int groups = B * T * n_kv_head * 2;
  hipLaunchKernelGGL(kv_append_fp8_kernel, dim3((groups * 16 + 255) / 256), dim3(256), 0, s,
                     static_cast<const bf16*>(k_new), ldk, static_cast<const bf16*>(v_new), ldv,
                     static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), k_scale, v_scale, pos, T, C,
                     n_kv_head, D, groups);
}
