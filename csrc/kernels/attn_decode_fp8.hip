// KV cache and decode attention with e4m3 caches: the fp8 forms of attn_decode.hip.
//
// Format: K and V bytes uint8 [B][C][n_kv_head*D] (OCP e4m3), scales fp32 [B][n_kv_head][C], one
// power-of-two scale per (position, KV head) by the rule of models/params.py quantize_fp8. An e4m3
// value times a power of two is a bf16 value, so what the kernel multiplies is exactly the
// dequantised bf16 row.
//
// attn_decode_fp8: the grid, the chunk rule (attn_decode_chunk), the ticketed order-independent
// merge, the partial format and the workspace sizes are those of the bf16 kernel; read that file
// for them. What differs:
//  * A stage holds the same KTS keys as the bf16 kernel's, in half the bytes (16 KB per operand),
//    plus the stage's K and V scales (KTS fp32 each), which a wave fetches for its own 64 keys with
//    two 4-byte LDS-DMA instructions. The ring keeps the bf16 kernel's two buffers (68 KB): a ring
//    of four with three stages in flight was measured and is slower (52.7 us against 49.3 us at
//    Llama-3-8B, B = 8, T = 1, P = 8192), so bytes in flight are not what limits this kernel.
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
#include <algorithm>

#include "common.h"
#include "kernels.h"

#include "attention_impl.h"

namespace {

using dls_attn::BoolC;
using dls_attn::lds_bf16x4;
using dls_attn::raw_barrier;
using dls_attn::swz;
using dls_attn::wait_vm;
using dls_attn::xlane;

typedef __attribute__((address_space(3))) void lds_void;

template <int D, int NG_>
struct Dec8Cfg {
  static constexpr int NG = NG_;                 // 16-wide query column groups
  static constexpr int KS = D == 64 ? 4 : 2;     // waves: each takes 64 keys of a stage
  static constexpr int KT = 64;
  static constexpr int KTS = KT * KS;            // keys per stage, as DecCfg (attn_decode_chunk)
  static constexpr int RB = D;                   // bytes per K/V row
  static constexpr int CH = D / 16;              // 16-B chunks per row
  static constexpr int ROWS_PER_INSTR = 1024 / RB;
  static constexpr int INSTR = KTS / ROWS_PER_INSTR;  // per operand per stage
  static constexpr int PW = 2 * INSTR / KS;           // per wave per stage (K and V)
  static constexpr int TILE_BYTES = KTS * RB;
  static constexpr int KSC_OFF = 2 * TILE_BYTES;      // K scales [KTS] fp32, then V scales
  static constexpr int VSC_OFF = KSC_OFF + KTS * 4;
  static constexpr int BUF_BYTES = VSC_OFF + KTS * 4;
  static constexpr int NQK = D / 32;
  static constexpr int ND = D / 16;
  static constexpr int REC = ND * 4 + 2;   // wave merge, floats per lane and group: o, m, l
  static constexpr int MERGE_BYTES = (KS - 1) * NG * 64 * REC * 4;
  static constexpr int SMEM = 2 * BUF_BYTES > MERGE_BYTES ? 2 * BUF_BYTES : MERGE_BYTES;
  // one chunk's published partial: DecCfg's (the d a lane's o stands for differs, the bytes do not)
  static constexpr int ML_OFF = NG * ND * 1024;
  static constexpr int CHUNK_BYTES = ML_OFF + NG * 512;
  static_assert(PW * KS == 2 * INSTR && INSTR % PW == 0, "DMA split");
  static_assert(SMEM <= 163840, "LDS budget");
};

template <int D>
constexpr int kDec8Threads = 64 * Dec8Cfg<D, 1>::KS;

// two e4m3 bytes (the low or the high half of w) -> two bf16, exact (every e4m3 value is a bf16 value)
template <bool HI>
__device__ __forceinline__ bf16x2 cvt2(uint32_t w) {
  return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);  // v_cvt_scalef32_pk_bf16_fp8, scale 1
}

template <int D, int NG>
__global__ __launch_bounds__(kDec8Threads<D>) void attn_decode_fp8_kernel(
    const bf16* __restrict__ Q, int ldq, const uint8_t* __restrict__ Kc, const uint8_t* __restrict__ Vc,
    const float* __restrict__ Ks, const float* __restrict__ Vs, bf16* __restrict__ O, int ldo,
    const int* __restrict__ pos, int T, int C, int KC, int n_head, int n_kv_head, float scale_log2,
    float* __restrict__ part, int* __restrict__ cnt) {
  using Cf = Dec8Cfg<D, NG>;
  __shared__ __attribute__((aligned(16))) char smem[Cf::SMEM];
  const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int hg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int p0 = max(pos[b], 0);
  const int n_keys = min(p0 + T, C);
  const int nact = min((n_keys + KC - 1) / KC, (int)gridDim.x);
  if (c >= nact) return;  // no key of this sequence in the chunk: no ticket either
  const int k_lo = c * KC, k_hi = min(k_lo + KC, n_keys);  // k_lo < k_hi
  const int rep = n_head / n_kv_head, ncol = rep * T;

  // LDS-DMA as attn_decode.hip: instruction j of this wave covers rows r0 .. r0+ROWS_PER_INSTR-1
  // of operand op; then the scales of the wave's own 64 keys, one fp32 per lane
  const size_t ld = (size_t)n_kv_head * D;
  const int dop = hg * Cf::PW / Cf::INSTR;  // 0 = K, 1 = V
  const uint8_t* dbase = (dop == 0 ? Kc : Vc) + (size_t)b * C * ld + kvh * D;
  const size_t sbase = ((size_t)b * n_kv_head + kvh) * C;
  const int lrow = lane / Cf::CH, lch = lane % Cf::CH;
  auto issue = [&](int t) {
    char* buf = smem + (t & 1) * Cf::BUF_BYTES;
    const int key0 = k_lo + t * Cf::KTS;
#pragma unroll
    for (int j = 0; j < Cf::PW; ++j) {
      const int r0 = ((hg * Cf::PW + j) % Cf::INSTR) * Cf::ROWS_PER_INSTR;
      if (key0 + r0 / Cf::KT * Cf::KT >= k_hi) continue;  // wave-uniform: that wave tile is not computed
      const int row = r0 + lrow;
      const int gch = lch ^ swz(row, Cf::CH - 1);
      const uint8_t* src = dbase + (size_t)min(key0 + row, k_hi - 1) * ld + gch * 16;
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)(buf + dop * Cf::TILE_BYTES + r0 * Cf::RB), 16,
                                       0, 0);
    }
    if (key0 + hg * Cf::KT < k_hi) {  // wave-uniform; the index is clamped as the rows are
      const size_t si = sbase + min(key0 + hg * Cf::KT + lane, k_hi - 1);
      __builtin_amdgcn_global_load_lds((const void*)(Ks + si), (lds_void*)(buf + Cf::KSC_OFF + hg * Cf::KT * 4), 4, 0,
                                       0);
      __builtin_amdgcn_global_load_lds((const void*)(Vs + si), (lds_void*)(buf + Cf::VSC_OFF + hg * Cf::KT * 4), 4, 0,
                                       0);
    }
  };

  const int nst = (k_hi - k_lo + Cf::KTS - 1) / Cf::KTS;
  issue(0);  // before anything else waits on memory

  // Q^T as the B operand: lane holds column ng*16 + li, elements 32*ks + 8*g + j
  bf16x8 qf[NG][Cf::NQK];
  int qlim[NG];  // the last key the column's query sees
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    const int j = min(ng * 16 + li, ncol - 1);
    const int r = j / T, t = j - r * T;
    qlim[ng] = p0 + t;
    const bf16* qrow = Q + ((size_t)b * T + t) * ldq + (kvh * rep + r) * D;
#pragma unroll
    for (int ks = 0; ks < Cf::NQK; ++ks) qf[ng][ks] = *reinterpret_cast<const bf16x8*>(qrow + 32 * ks + 8 * g);
  }

  // o[ng][2*dp + par][i] <-> d = 32*dp + 2*(4g + i) + par of column ng*16 + li
  f32x4 o[NG][Cf::ND];
  float m_run[NG], l_run[NG];
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    m_run[ng] = -INFINITY;
    l_run[ng] = 0.f;
#pragma unroll
    for (int i = 0; i < Cf::ND; ++i) o[ng][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // one 64-key wave tile: S^T = K Q^T, online softmax, O^T += V^T P^T for NG column groups
  auto stage = [&](int t, int key0, auto mask_c) {
    const char* buf = smem + (t & 1) * Cf::BUF_BYTES;
    const char* kb = buf + hg * Cf::KT * Cf::RB;
    const char* vb = kb + Cf::TILE_BYTES;
    f32x4 s[NG][4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) s[ng][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int row = 16 * n + li;
#pragma unroll
      for (int ks = 0; ks < Cf::NQK; ++ks) {
        const int ch = 2 * ks + (g >> 1);
        const u32x2 kw =
            *reinterpret_cast<const u32x2*>(kb + row * Cf::RB + ((ch ^ swz(row, Cf::CH - 1)) << 4) + (g & 1) * 8);
        const bf16x2 k0 = cvt2<false>(kw[0]), k1 = cvt2<true>(kw[0]);
        const bf16x2 k2 = cvt2<false>(kw[1]), k3 = cvt2<true>(kw[1]);
        const bf16x8 kf = {k0[0], k0[1], k1[0], k1[1], k2[0], k2[1], k3[0], k3[1]};
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) s[ng][n] = mfma16x16x32(kf, qf[ng][ks], s[ng][n]);
      }
    }
    // scores s[ng][n][i] <-> key key0 + 16n + 4g + i of column ng*16 + li; the scales of those keys
    f32x4 ksc[4], vsc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      ksc[n] = *reinterpret_cast<const f32x4*>(buf + Cf::KSC_OFF + (hg * Cf::KT + 16 * n + 4 * g) * 4);
      vsc[n] = *reinterpret_cast<const f32x4*>(buf + Cf::VSC_OFF + (hg * Cf::KT + 16 * n + 4 * g) * 4);
    }
    bf16x8 pf[NG][2];
#pragma unroll
    for (int ng = 0; ng < NG; ++ng) {
#pragma unroll
      for (int n = 0; n < 4; ++n) s[ng][n] *= ksc[n];
      if constexpr (decltype(mask_c)::value) {
        const int lim = min(qlim[ng], k_hi - 1);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (key0 + 16 * n + 4 * g + i > lim) s[ng][n][i] = -INFINITY;
      }
      float mx = fmaxf(fmaxf(s[ng][0][0], s[ng][0][1]), fmaxf(s[ng][0][2], s[ng][0][3]));
#pragma unroll
      for (int n = 1; n < 4; ++n)
        mx = fmaxf(mx, fmaxf(fmaxf(s[ng][n][0], s[ng][n][1]), fmaxf(s[ng][n][2], s[ng][n][3])));
      mx = xlane<true, 16>(mx);
      mx = xlane<true, 32>(mx);
      // a column may see no key of a tile (a later chunk's first keys are the newer tokens): the
      // clamp keeps its exponents at -inf and its sum at zero
      const float m_new = fmaxf(fmaxf(m_run[ng], mx), -1e30f);
      const float alpha = __builtin_amdgcn_exp2f((m_run[ng] - m_new) * scale_log2);
      const float mc = m_new * scale_log2;
      float sum = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = __builtin_amdgcn_exp2f(fmaf(s[ng][n][i], scale_log2, -mc));
          sum += e;
          pf[ng][n >> 1][4 * (n & 1) + i] = f2bf(e * vsc[n][i]);  // a masked key: 0 * a valid key's scale
        }
      sum = xlane<false, 16>(sum);
      sum = xlane<false, 32>(sum);
      l_run[ng] = l_run[ng] * alpha + sum;
      m_run[ng] = m_new;
#pragma unroll
      for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] *= alpha;
    }
    // O^T += V^T P^T ; V^T fragment element j <-> key 32ks + 16(j>>2) + 4g + (j&3). The lane's
    // read address is row 32ks (+16) + 4g + q4, bytes 32dp + 8*p4 .. +7; it receives byte pair li
    // (d = 32dp + 2li, +1) of rows 32ks (+16) + 4g + 0..3.
    const int q4 = li >> 2, p4 = li & 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int dp = 0; dp < Cf::ND / 2; ++dp) {
        const int ch = 2 * dp + (p4 >> 1);
        const int row0 = 32 * ks + 4 * g + q4;
        const int row1 = row0 + 16;
        const lds_bf16x4* a0 =
            (const lds_bf16x4*)(vb + row0 * Cf::RB + ((ch ^ swz(row0, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const lds_bf16x4* a1 =
            (const lds_bf16x4*)(vb + row1 * Cf::RB + ((ch ^ swz(row1, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
        const u32x2 wl = *reinterpret_cast<const u32x2*>(&lo), wh = *reinterpret_cast<const u32x2*>(&hi);
        // a word is [key a: d0 d1 | key a+1: d0 d1]; after the permute [a d0, a+1 d0 | a d1, a+1 d1]
        const uint32_t w0 = __builtin_amdgcn_perm(wl[0], wl[0], 0x03010200u);
        const uint32_t w1 = __builtin_amdgcn_perm(wl[1], wl[1], 0x03010200u);
        const uint32_t w2 = __builtin_amdgcn_perm(wh[0], wh[0], 0x03010200u);
        const uint32_t w3 = __builtin_amdgcn_perm(wh[1], wh[1], 0x03010200u);
        {
          const bf16x2 e0 = cvt2<false>(w0), e1 = cvt2<false>(w1), e2 = cvt2<false>(w2), e3 = cvt2<false>(w3);
          const bf16x8 vf = {e0[0], e0[1], e1[0], e1[1], e2[0], e2[1], e3[0], e3[1]};
#pragma unroll
          for (int ng = 0; ng < NG; ++ng) o[ng][2 * dp] = mfma16x16x32(vf, pf[ng][ks], o[ng][2 * dp]);
        }
        {
          const bf16x2 e0 = cvt2<true>(w0), e1 = cvt2<true>(w1), e2 = cvt2<true>(w2), e3 = cvt2<true>(w3);
          const bf16x8 vf = {e0[0], e0[1], e1[0], e1[1], e2[0], e2[1], e3[0], e3[1]};
#pragma unroll
          for (int ng = 0; ng < NG; ++ng) o[ng][2 * dp + 1] = mfma16x16x32(vf, pf[ng][ks], o[ng][2 * dp + 1]);
        }
      }
    }
  };

  for (int t = 0; t < nst; ++t) {
    wait_vm<0>();
    raw_barrier();
    if (t + 1 < nst) issue(t + 1);  // into the buffer everyone finished in t-1
    const int key0 = k_lo + t * Cf::KTS + hg * Cf::KT;
    if (key0 < k_hi) {  // wave-uniform
      const bool masked = key0 + Cf::KT > k_hi || key0 + Cf::KT - 1 > p0;
      if (masked) stage(t, key0, BoolC<true>{});
      else stage(t, key0, BoolC<false>{});
    }
  }

  // merge the KS wave chains in one LDS exchange; wave 0 holds the result (as attn_decode.hip)
  auto wave_merge = [&]() {
    __syncthreads();  // every wave is done with what the LDS held
    float* mg = reinterpret_cast<float*>(smem);
    constexpr int REC = Cf::REC, LN = 64;
    if (hg > 0) {
      float* r = mg + (hg - 1) * NG * REC * LN + lane;
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) {
#pragma unroll
        for (int dn = 0; dn < Cf::ND; ++dn)
#pragma unroll
          for (int i = 0; i < 4; ++i) r[(ng * REC + dn * 4 + i) * LN] = o[ng][dn][i];
        r[(ng * REC + Cf::ND * 4) * LN] = m_run[ng];
        r[(ng * REC + Cf::ND * 4 + 1) * LN] = l_run[ng];
      }
    }
    __syncthreads();
    if (hg == 0) {
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) {
        float mo[Cf::KS - 1], lo_[Cf::KS - 1];
        float mm = m_run[ng];
#pragma unroll
        for (int h2 = 0; h2 < Cf::KS - 1; ++h2) {
          const float* r = mg + (h2 * NG + ng) * REC * LN + lane;
          mo[h2] = r[Cf::ND * 4 * LN];
          lo_[h2] = r[(Cf::ND * 4 + 1) * LN];
          mm = fmaxf(mm, mo[h2]);
        }
        mm = fmaxf(mm, -1e30f);
        const float a0 = __builtin_amdgcn_exp2f((m_run[ng] - mm) * scale_log2);
        l_run[ng] *= a0;
#pragma unroll
        for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] *= a0;
#pragma unroll
        for (int h2 = 0; h2 < Cf::KS - 1; ++h2) {
          const float* r = mg + (h2 * NG + ng) * REC * LN + lane;
          const float a1 = __builtin_amdgcn_exp2f((mo[h2] - mm) * scale_log2);
          l_run[ng] += lo_[h2] * a1;
#pragma unroll
          for (int dn = 0; dn < Cf::ND; ++dn)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[ng][dn][i] += r[(dn * 4 + i) * LN] * a1;
        }
        m_run[ng] = mm;
      }
    }
  };
  wave_merge();

  // O[b*T + t][(kvh*rep + r)*D + 32dp + 8g + 2i + par] of column j = r*T + t = ng*16 + li
  auto store = [&](int ng, int dp, const f32x4& even, const f32x4& odd, float l) {
    const int j = ng * 16 + li;
    if (j >= ncol) return;
    const int r = j / T, t = j - r * T;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = f2bf(even[i] * inv);
      v[2 * i + 1] = f2bf(odd[i] * inv);
    }
    *reinterpret_cast<bf16x8*>(O + ((size_t)b * T + t) * ldo + (kvh * rep + r) * D + 32 * dp + 8 * g) = v;
  };

  if (nact == 1) {
    if (hg != 0) return;
#pragma unroll
    for (int ng = 0; ng < NG; ++ng)
#pragma unroll
      for (int dp = 0; dp < Cf::ND / 2; ++dp) store(ng, dp, o[ng][2 * dp], o[ng][2 * dp + 1], l_run[ng]);
    return;
  }

  // publish this chunk's (o, m, l), draw a ticket, the last arriver merges: attn_decode.hip
  const size_t head_id = (size_t)b * n_kv_head + kvh;
  float* pp = part + head_id * gridDim.x * (Cf::CHUNK_BYTES / 4);
  const auto rp = __builtin_amdgcn_make_buffer_rsrc(pp, 0, 0x7fffffff, 0x00020000);
  if (hg == 0) {
#pragma unroll
    for (int ng = 0; ng < NG; ++ng) {
#pragma unroll
      for (int dn = 0; dn < Cf::ND; ++dn)
        __builtin_amdgcn_raw_buffer_store_b128(
            u32x4{__float_as_uint(o[ng][dn][0]), __float_as_uint(o[ng][dn][1]), __float_as_uint(o[ng][dn][2]),
                  __float_as_uint(o[ng][dn][3])},
            rp, c * Cf::CHUNK_BYTES + ((ng * Cf::ND + dn) * 64 + lane) * 16, 0, 16);
      __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(m_run[ng]), __float_as_uint(l_run[ng])}, rp,
                                            c * Cf::CHUNK_BYTES + Cf::ML_OFF + (ng * 64 + lane) * 8, 0, 16);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-through stores landed
  __syncthreads();
  int* flag = reinterpret_cast<int*>(smem);
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(cnt + head_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == nact - 1;
    if (last) __hip_atomic_store(cnt + head_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    flag[0] = last;
  }
  __syncthreads();
  if (!flag[0]) return;  // block-uniform
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    m_run[ng] = -INFINITY;
    l_run[ng] = 0.f;
#pragma unroll
    for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  constexpr int U = NG == 1 ? 4 : NG == 2 ? 2 : 1;  // chunks in flight together, as attn_decode.hip
  for (int c0 = hg; c0 < nact; c0 += Cf::KS * U) {
    f32x4 o2[U][NG][Cf::ND];
    float m2[U][NG], l2[U][NG];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c2 = min(c0 + u * Cf::KS, nact - 1);
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) {
#pragma unroll
        for (int dn = 0; dn < Cf::ND; ++dn) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
              rp, c2 * Cf::CHUNK_BYTES + ((ng * Cf::ND + dn) * 64 + lane) * 16, 0, 16);
          o2[u][ng][dn] =
              f32x4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
        }
        const u32x2 ml =
            __builtin_amdgcn_raw_buffer_load_b64(rp, c2 * Cf::CHUNK_BYTES + Cf::ML_OFF + (ng * 64 + lane) * 8, 0, 16);
        m2[u][ng] = __uint_as_float(ml[0]);
        l2[u][ng] = __uint_as_float(ml[1]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = c0 + u * Cf::KS < nact;
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) {
        const float mm = fmaxf(m_run[ng], m2[u][ng]);  // m2 >= -1e30
        const float a0 = __builtin_amdgcn_exp2f((m_run[ng] - mm) * scale_log2);
        const float a1 = in ? __builtin_amdgcn_exp2f((m2[u][ng] - mm) * scale_log2) : 0.f;
        l_run[ng] = l_run[ng] * a0 + l2[u][ng] * a1;
        m_run[ng] = mm;
#pragma unroll
        for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] = o[ng][dn] * a0 + o2[u][ng][dn] * a1;
      }
    }
  }
  wave_merge();
  if (hg != 0) return;
#pragma unroll
  for (int ng = 0; ng < NG; ++ng)
#pragma unroll
    for (int dp = 0; dp < Cf::ND / 2; ++dp) store(ng, dp, o[ng][2 * dp], o[ng][2 * dp + 1], l_run[ng]);
}

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

template <int D, int NG>
void launch_decode8(const DecodeArgs& a, int KC, hipStream_t s) {
  using Cf = Dec8Cfg<D, NG>;
  dim3 grid((a.C + KC - 1) / KC, a.n_kv_head, a.B), block(64 * Cf::KS);
  hipLaunchKernelGGL((attn_decode_fp8_kernel<D, NG>), grid, block, 0, s, static_cast<const bf16*>(a.q), a.ldq,
                     static_cast<const uint8_t*>(a.k_cache), static_cast<const uint8_t*>(a.v_cache), a.k_scale,
                     a.v_scale, static_cast<bf16*>(a.o), a.ldo, a.pos, a.T, a.C, KC, a.n_head, a.n_kv_head,
                     a.scale * 1.4426950408889634f, static_cast<float*>(a.part), static_cast<int*>(a.cnt));
}

template <int D>
void launch_decode8_d(const DecodeArgs& a, int ng, int KC, hipStream_t s) {
  switch (ng) {
    case 1: launch_decode8<D, 1>(a, KC, s); break;
    case 2: launch_decode8<D, 2>(a, KC, s); break;
    case 3: launch_decode8<D, 3>(a, KC, s); break;
    default: launch_decode8<D, 4>(a, KC, s); break;
  }
}

}  // namespace

void launch_attn_decode_fp8(const DecodeArgs& a, hipStream_t s) {
  const int KC = a.chunk > 0 ? a.chunk : attn_decode_chunk(a.B, a.C, a.n_kv_head, a.D);
  const int ng = (a.n_head / a.n_kv_head * a.T + 15) / 16;
  if (a.D == 64) launch_decode8_d<64>(a, ng, KC, s);
  else launch_decode8_d<128>(a, ng, KC, s);
}

void launch_kv_append_fp8(const void* k_new, int ldk, const void* v_new, int ldv, void* k_cache, void* v_cache,
                          float* k_scale, float* v_scale, const int* pos, int B, int T, int C, int n_kv_head, int D,
                          hipStream_t s) {
  const int groups = B * T * n_kv_head * 2;
  hipLaunchKernelGGL(kv_append_fp8_kernel, dim3((groups * 16 + 255) / 256), dim3(256), 0, s,
                     static_cast<const bf16*>(k_new), ldk, static_cast<const bf16*>(v_new), ldv,
                     static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), k_scale, v_scale, pos, T, C,
                     n_kv_head, D, groups);
}
