// What the attention kernels over an e4m3 KV cache do with the bytes in LDS, shared by the decode
// kernel (attn_decode_fp8.hip) and the prompt-chunk kernel (attn_chunk_fp8.hip): the conversion of
// a byte pair and the cache-format traits `Fp8Cache` (the `Cache` of attn_decode_impl.h; the two
// fragment functions only need RB, CH, NG and ND of the configuration they are given).
#pragma once
#include "common.h"
#include "kernels.h"

#include "attention_impl.h"

namespace dls_fp8 {

using dls_attn::swz;

// two e4m3 bytes (the low or the high half of w) -> two bf16, exact (every e4m3 value is a bf16 value)
template <bool HI>
__device__ __forceinline__ bf16x2 cvt2(uint32_t w) {
  return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);  // v_cvt_scalef32_pk_bf16_fp8, scale 1
}

// o[ng][2*dp + par][i] <-> d = 32*dp + 2*(4g + i) + par of column ng*16 + li
struct Fp8Cache {
  using Elem = uint8_t;
  static constexpr int SCALE_BYTES = 4;
  struct Operands {
    const uint8_t *K, *V;
    const float *Ks, *Vs;
    template <class F>
    void each(F f) const { f(K, V, Ks, Vs); }
  };
  static Operands operands(const DecodeArgs& a) {
    return {static_cast<const uint8_t*>(a.k_cache), static_cast<const uint8_t*>(a.v_cache), a.k_scale, a.v_scale};
  }

  template <class Cf>
  static __device__ __forceinline__ bf16x8 k_frag(const char* kb, int row, int ks, int g) {
    const int ch = 2 * ks + (g >> 1);
    const u32x2 kw =
        *reinterpret_cast<const u32x2*>(kb + row * Cf::RB + ((ch ^ swz(row, Cf::CH - 1)) << 4) + (g & 1) * 8);
    const bf16x2 k0 = cvt2<false>(kw[0]), k1 = cvt2<true>(kw[0]);
    const bf16x2 k2 = cvt2<false>(kw[1]), k3 = cvt2<true>(kw[1]);
    return {k0[0], k0[1], k1[0], k1[1], k2[0], k2[1], k3[0], k3[1]};
  }

  // lo, hi: byte pair li (d = 32dp + 2li, +1) of four keys each
  template <class Cf>
  static __device__ __forceinline__ void pv(const bf16x4& lo, const bf16x4& hi, int dp, int ks,
                                            const bf16x8 (&pf)[Cf::NG][2], f32x4 (&o)[Cf::NG][Cf::ND]) {
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
      for (int ng = 0; ng < Cf::NG; ++ng) o[ng][2 * dp] = mfma16x16x32(vf, pf[ng][ks], o[ng][2 * dp]);
    }
    {
      const bf16x2 e0 = cvt2<true>(w0), e1 = cvt2<true>(w1), e2 = cvt2<true>(w2), e3 = cvt2<true>(w3);
      const bf16x8 vf = {e0[0], e0[1], e1[0], e1[1], e2[0], e2[1], e3[0], e3[1]};
#pragma unroll
      for (int ng = 0; ng < Cf::NG; ++ng) o[ng][2 * dp + 1] = mfma16x16x32(vf, pf[ng][ks], o[ng][2 * dp + 1]);
    }
  }
};

}  // namespace dls_fp8
