// Prompt-chunk attention straight over the e4m3 KV cache: the T new queries of every sequence
// (1 <= T <= 1024) against cache rows 0 .. pos[b]+t, with K and V read as the bytes they are stored
// as (uint8 [B][C][n_kv_head*D], scales fp32 [B][n_kv_head][C]). No dequantise pass, no workspace.
//
// Work split. A query tile is QT consecutive tokens of one sequence for ALL rep = n_head/n_kv_head
// query heads of one KV head, QT the largest power of two with rep*QT <= 64. Its rep*QT query rows
// are the operand columns of the swapped-operand form of attn_decode_impl.h (S^T = K Q^T,
// O^T += V^T P^T; column j = r*QT + t is token t0 + t of head kvh*rep + r), NG = ceil(rep*QT/16)
// column groups per wave (3 or 4: rep*QT > 32 by the choice of QT). Every K and V fragment read from
// LDS feeds NG MFMAs, so the cache bytes are staged once per KV head and tile, not once per query
// head. A workgroup holds NW query tiles x KS key groups of waves that share one staged stage of
// 64*KS keys: wave (wq, hg) runs tile grp*NW + wq over keys 64*hg .. +63 of every stage with an
// online-softmax chain of its own, and the KS chains of a tile are merged through LDS once at the
// end. Grid (ceil(ceil(T/QT)/NW), n_kv_head, B), the heaviest tiles first; it depends on the shapes
// alone and pos[b] is read here, so a captured launch follows a growing, ragged batch. No key
// split across workgroups, no tickets.
//
// Keys. Tile t0 walks keys 0 .. k_hi - 1, k_hi = min(pos[b] + min(t0 + QT, T), C); the workgroup
// stages up to the k_hi of its last tile. K/V bytes and the stage's K and V scales arrive by
// LDS-DMA into a two-buffer ring (the fp8 decode kernel's stage format); DMA rows and the scale
// index are clamped to the workgroup's last valid key, a 64-key wave tile without a valid key is
// neither fetched nor computed, so rows and scales at or past pos[b]+T never reach arithmetic.
// Only wave tiles that reach past pos[b]+t0 (or past the tile's k_hi) carry the per-column mask
// key > pos[b]+t0+t. Rows a tile stages but does not see (the chunk's own later tokens) enter the
// second MFMA as 0 x v: V rows below pos[b]+T must be finite, as ops.attention_chunk states.
//
// Arithmetic is Fp8Cache's (attn_fp8_frag.h): K fragments converted in registers at scale 1, V^T
// through the 16-bit transposed read and one v_perm_b32 per word into two MFMAs, the K scale on the
// fp32 score of its key and the V scale on p before p is rounded to bf16 (exact: powers of two).
// (NW, KS) per D: profiles/chunk_fp8/ (resource remarks of every instance, kernel A/B).
#include "common.h"
#include "kernels.h"

#include "attn_fp8_frag.h"

namespace {

using dls_attn::BoolC;
using dls_attn::lds_bf16x4;
using dls_attn::raw_barrier;
using dls_attn::swz;
using dls_attn::wait_vm;
using dls_attn::xlane;
using dls_fp8::Fp8Cache;

typedef __attribute__((address_space(3))) void lds_void;

template <int D, int NG_, int NW_, int KS_>
struct ChunkCfg {
  static constexpr int NG = NG_;             // 16-wide query column groups
  static constexpr int NW = NW_;             // query tiles per workgroup
  static constexpr int KS = KS_;             // key groups: each takes 64 keys of a stage
  static constexpr int NWV = NW * KS;        // waves
  static constexpr int KT = 64;
  static constexpr int KTS = KT * KS;        // keys per stage
  static constexpr int RB = D;               // bytes per K/V row
  static constexpr int CH = RB / 16;         // 16-B chunks per row
  static constexpr int NVT = RB / 32;        // pairs of transposed V reads per row
  static constexpr int ROWS_PER_INSTR = 1024 / RB;
  static constexpr int INSTR = KTS / ROWS_PER_INSTR;  // per operand per stage
  static constexpr int PW = 2 * INSTR / NWV;          // per wave per stage (K and V)
  static constexpr int TILE_BYTES = KTS * RB;
  static constexpr int KSC_OFF = 2 * TILE_BYTES;      // K scales [KTS], then V scales
  static constexpr int VSC_OFF = KSC_OFF + KTS * 4;
  static constexpr int BUF_BYTES = VSC_OFF + KTS * 4;
  static constexpr int NQK = D / 32;
  static constexpr int ND = D / 16;
  static constexpr int REC = ND * 4 + 2;     // wave merge, floats per lane and group: o, m, l
  static constexpr int MERGE_BYTES = NW * (KS - 1) * NG * 64 * REC * 4;
  static constexpr int SMEM = 2 * BUF_BYTES > MERGE_BYTES ? 2 * BUF_BYTES : MERGE_BYTES;
  static_assert(PW >= 1 && PW * NWV == 2 * INSTR && INSTR % PW == 0, "DMA split");
  static_assert(SMEM <= 163840, "LDS budget");
};

template <int D, int NG, int NW, int KS>
__global__ __launch_bounds__(64 * NW * KS) void attn_chunk_fp8_kernel(
    const bf16* __restrict__ Q, int ldq, const uint8_t* __restrict__ Kc, const uint8_t* __restrict__ Vc,
    const float* __restrict__ Ksc, const float* __restrict__ Vsc, bf16* __restrict__ O, int ldo,
    const int* __restrict__ pos, int T, int C, int n_head, int n_kv_head, float scale_log2, int qt_log2) {
  using Cf = ChunkCfg<D, NG, NW, KS>;
  __shared__ __attribute__((aligned(16))) char smem[Cf::SMEM];
  const int kvh = blockIdx.y, b = blockIdx.z;
  const int grp = gridDim.x - 1 - blockIdx.x;  // heaviest query tiles first
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wv / KS, hg = wv % KS;
  const int g = lane >> 4, li = lane & 15;
  const int QT = 1 << qt_log2;
  const int p0 = min(max(pos[b], 0), C);
  const int rep = n_head / n_kv_head, ncol = rep << qt_log2;
  // this wave's tile (one past the chunk in the last workgroup: no key, no store) and the
  // workgroup's last key, which bounds what is staged
  const int t0 = (grp * NW + wq) * QT;
  const int k_hi = t0 < T ? min(p0 + min(t0 + QT, T), C) : 0;
  const int k_stage = min(p0 + min((grp + 1) * NW * QT, T), C);  // >= 1

  // LDS-DMA: instruction j of this wave covers rows r0 .. r0+ROWS_PER_INSTR-1 of operand dop (a
  // wave's instructions all belong to one operand); the waves of tile 0 also fetch the scales of
  // their 64 keys, one fp32 per lane, with the rows' skip and the rows' clamp
  const size_t ld = (size_t)n_kv_head * D;
  const int dop = wv * Cf::PW / Cf::INSTR;  // 0 = K, 1 = V
  const uint8_t* dbase = (dop == 0 ? Kc : Vc) + (size_t)b * C * ld + kvh * D;
  const size_t sbase = ((size_t)b * n_kv_head + kvh) * C;
  const int lrow = lane / Cf::CH, lch = lane % Cf::CH;
  auto issue = [&](int t) {
    char* buf = smem + (t & 1) * Cf::BUF_BYTES;
    const int key0 = t * Cf::KTS;
#pragma unroll
    for (int j = 0; j < Cf::PW; ++j) {
      const int r0 = ((wv * Cf::PW + j) % Cf::INSTR) * Cf::ROWS_PER_INSTR;
      if (key0 + r0 / Cf::KT * Cf::KT >= k_stage) continue;  // wave-uniform: no tile computes that wave tile
      const int row = r0 + lrow;
      const int gch = lch ^ swz(row, Cf::CH - 1);
      const uint8_t* src = dbase + (size_t)min(key0 + row, k_stage - 1) * ld + gch * 16;
      char* dst = buf + dop * Cf::TILE_BYTES + r0 * Cf::RB;
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)dst, 16, 0, 0);
    }
    if (wq == 0 && key0 + hg * Cf::KT < k_stage) {  // wave-uniform
      const size_t si = sbase + min(key0 + hg * Cf::KT + lane, k_stage - 1);
      __builtin_amdgcn_global_load_lds((const void*)(Ksc + si), (lds_void*)(buf + Cf::KSC_OFF + hg * Cf::KT * 4), 4,
                                       0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(Vsc + si), (lds_void*)(buf + Cf::VSC_OFF + hg * Cf::KT * 4), 4,
                                       0, 0);
    }
  };

  const int nst = (k_stage + Cf::KTS - 1) / Cf::KTS;
  issue(0);  // before anything else waits on memory

  // Q^T as the B operand: lane holds column ng*16 + li, elements 32*ks + 8*g + j. A column past
  // the tile's rep*QT, or a token past the chunk, repeats a valid one and is never stored.
  bf16x8 qf[NG][Cf::NQK];
  int qlim[NG];  // the last key the column's query sees
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    const int j = min(ng * 16 + li, ncol - 1);
    const int r = j >> qt_log2, tok = min(t0 + (j & (QT - 1)), T - 1);
    qlim[ng] = p0 + tok;
    const bf16* qrow = Q + ((size_t)b * T + tok) * ldq + (kvh * rep + r) * D;
#pragma unroll
    for (int ks = 0; ks < Cf::NQK; ++ks) qf[ng][ks] = *reinterpret_cast<const bf16x8*>(qrow + 32 * ks + 8 * g);
  }

  // o[ng][2*dp + par][i] <-> d = 32*dp + 2*(4g + i) + par of column ng*16 + li (Fp8Cache::pv)
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
        const bf16x8 kf = Fp8Cache::k_frag<Cf>(kb, row, ks, g);
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) s[ng][n] = mfma16x16x32(kf, qf[ng][ks], s[ng][n]);
      }
    }
    // scores s[ng][n][i] <-> key key0 + 16n + 4g + i of column ng*16 + li; the K and the V scales of
    // those sixteen keys are eight 16-byte LDS reads
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
      // a column may see no key of a wave tile (the tile's first tokens against its last keys):
      // the clamp keeps its exponents at -inf and its sum at zero
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
    // read address is row 32ks (+16) + 4g + q4, bytes 32dx + 8*p4 .. +7; it receives the 16-bit
    // element li (a byte pair) of those 32 bytes from rows 32ks (+16) + 4g + 0..3.
    const int q4 = li >> 2, p4 = li & 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int dx = 0; dx < Cf::NVT; ++dx) {
        const int ch = 2 * dx + (p4 >> 1);
        const int row0 = 32 * ks + 4 * g + q4;
        const int row1 = row0 + 16;
        const lds_bf16x4* a0 =
            (const lds_bf16x4*)(vb + row0 * Cf::RB + ((ch ^ swz(row0, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const lds_bf16x4* a1 =
            (const lds_bf16x4*)(vb + row1 * Cf::RB + ((ch ^ swz(row1, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
        Fp8Cache::pv<Cf>(lo, hi, dx, ks, pf, o);
      }
    }
  };

  for (int t = 0; t < nst; ++t) {
    wait_vm<0>();
    raw_barrier();
    if (t + 1 < nst) issue(t + 1);  // into the buffer everyone finished in t-1
    const int key0 = t * Cf::KTS + hg * Cf::KT;
    if (key0 < k_hi) {  // wave-uniform
      const bool masked = key0 + Cf::KT > k_hi || key0 + Cf::KT - 1 > p0 + t0;
      if (masked) stage(t, key0, BoolC<true>{});
      else stage(t, key0, BoolC<false>{});
    }
  }

  // merge the KS chains of every tile in one LDS exchange (field-major slabs); wave hg = 0 of the
  // tile holds the result
  if constexpr (KS > 1) {
    __syncthreads();  // every wave is done with what the LDS held
    float* mg = reinterpret_cast<float*>(smem) + wq * (KS - 1) * NG * Cf::REC * 64;
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
    if (hg > 0) return;
#pragma unroll
    for (int ng = 0; ng < NG; ++ng) {
      float mo[KS - 1], lo_[KS - 1];
      float mm = m_run[ng];
#pragma unroll
      for (int h2 = 0; h2 < KS - 1; ++h2) {
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
      for (int h2 = 0; h2 < KS - 1; ++h2) {
        const float* r = mg + (h2 * NG + ng) * REC * LN + lane;
        const float a1 = __builtin_amdgcn_exp2f((mo[h2] - mm) * scale_log2);
        l_run[ng] += lo_[h2] * a1;
#pragma unroll
        for (int dn = 0; dn < Cf::ND; ++dn)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[ng][dn][i] += r[(dn * 4 + i) * LN] * a1;
      }
    }
  }

  // lane (g, li) holds the eight consecutive d = 32*dx + 8*g .. +7 of its column: one 16-byte store
  // into row b*T + t0 + t, head kvh*rep + r
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    const int j = ng * 16 + li;
    const int r = j >> qt_log2, tok = t0 + (j & (QT - 1));
    if (j >= ncol || tok >= T) continue;
    const float inv = l_run[ng] > 0.f ? 1.f / l_run[ng] : 0.f;
    bf16* orow = O + ((size_t)b * T + tok) * ldo + (kvh * rep + r) * D + 8 * g;
#pragma unroll
    for (int dx = 0; dx < Cf::NVT; ++dx) {
      bf16x8 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = f2bf(o[ng][2 * dx][i] * inv);
        v[2 * i + 1] = f2bf(o[ng][2 * dx + 1][i] * inv);
      }
      *reinterpret_cast<bf16x8*>(orow + 32 * dx) = v;
    }
  }
}

// the largest power of two QT with rep * QT <= 64, as its log2
int tile_log2(int rep) {
  int l = 0;
  while ((rep << (l + 1)) <= 64) ++l;
  return l;
}

template <int D, int NG, int NW, int KS>
void launch_cfg(const ChunkFp8Args& a, int qt_log2, hipStream_t s) {
  const int nq = (a.T + (1 << qt_log2) - 1) >> qt_log2;
  dim3 grid((nq + NW - 1) / NW, a.n_kv_head, a.B), block(64 * NW * KS);
  hipLaunchKernelGGL((attn_chunk_fp8_kernel<D, NG, NW, KS>), grid, block, 0, s, static_cast<const bf16*>(a.q), a.ldq,
                     static_cast<const uint8_t*>(a.k_cache), static_cast<const uint8_t*>(a.v_cache), a.k_scale,
                     a.v_scale, static_cast<bf16*>(a.o), a.ldo, a.pos, a.T, a.C, a.n_head, a.n_kv_head,
                     a.scale * 1.4426950408889634f, qt_log2);
}

template <int D, int NG>
void launch_ng(const ChunkFp8Args& a, int qt_log2, hipStream_t s) {
  const int layout = attn_chunk_fp8_layout(a.B, a.T, a.n_head, a.n_kv_head, a.D, a.layout);
  if constexpr (D == 64) {  // four key groups at D = 128, NG = 4 spill to scratch: no such instance
    if (layout == 14) return launch_cfg<D, NG, 1, 4>(a, qt_log2, s);
  }
  if (layout == 22) launch_cfg<D, NG, 2, 2>(a, qt_log2, s);
  else launch_cfg<D, NG, 1, 2>(a, qt_log2, s);
}

template <int D>
void launch_d(const ChunkFp8Args& a, hipStream_t s) {
  const int rep = a.n_head / a.n_kv_head, ql = tile_log2(rep);
  if (((rep << ql) + 15) / 16 == 3) launch_ng<D, 3>(a, ql, s);  // rep*QT is in 33 .. 64
  else launch_ng<D, 4>(a, ql, s);
}

}  // namespace

const char* attn_chunk_fp8_refusal(int T, int n_head, int n_kv_head, int D) {
  if (T < 1 || T > 1024) return "needs 1 <= T <= 1024";
  if (n_kv_head < 1 || n_head < n_kv_head || n_head % n_kv_head) return "n_head must be a multiple of n_kv_head";
  if (n_head / n_kv_head > 64) return "takes at most 64 query heads per KV head";
  if (D != 64 && D != 128) return "head_dim must be 64 or 128";
  return nullptr;
}

int attn_chunk_fp8_layout(int B, int T, int n_head, int n_kv_head, int D, int layout) {
  if (layout == 12 || layout == 22 || (layout == 14 && D == 64)) return layout;
  // measured (profiles/chunk_fp8/kernel_layouts.txt): two tiles per workgroup never won by more
  // than the spread; at D = 64 four key groups halve the time while the grid leaves CUs idle
  // (GPT-2, Tc 256: 48 workgroups) and lose a fifth once it fills them (384)
  const long wgs = (long)((T + (1 << tile_log2(n_head / n_kv_head)) - 1) >> tile_log2(n_head / n_kv_head)) * n_kv_head * B;
  return D == 64 && wgs <= 256 ? 14 : 12;
}

void launch_attn_chunk_fp8(const ChunkFp8Args& a, hipStream_t s) {
  if (a.D == 64) launch_d<64>(a, s);
  else launch_d<128>(a, s);
}
