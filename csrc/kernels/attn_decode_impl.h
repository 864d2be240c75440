// Decode attention on MFMA, the kernel that attn_decode.hip (bf16 KV cache) and attn_decode_fp8.hip
// (e4m3 KV cache) instantiate — the step that extends every sequence by T <= 16 tokens against keys
// it already holds. One kernel template and one host dispatch; what a cache format states and
// does itself is listed at `Cache` below.
//
// Workgroup = one (key chunk of KC keys, KV head, sequence). Its query rows are the rep*T rows of
// the KV head's rep = n_head/n_kv_head query heads, packed as the 16-wide operand columns of the
// swapped-operand formulation of attention_impl.h (S^T = K Q^T, O^T += V^T P^T; column
// j = r*T + t is new token t of query head kvh*rep + r), NG = ceil(rep*T/16) column groups per
// wave: every K and V fragment is read from LDS once and used by NG MFMAs, so the K/V bytes are
// read once per KV head, not once per query head. The KS waves of the workgroup each walk 64 of a
// stage's keys with an online-softmax chain of their own and are merged through LDS.
//
// The grid (ceil(C/KC), n_kv_head, B) is fixed by the cache capacity C; the length comes from
// pos[b] in device memory, so a captured launch follows a growing sequence. With
// n_active = ceil((pos[b]+T)/KC) chunks holding keys, chunks at or past n_active exit at once.
// One active chunk normalises and stores. Otherwise every chunk publishes its unnormalised fp32
// (o, m, l) write-through (sc1), draws an agent-scope ticket of its (sequence, KV head), and the
// last arriver reloads ALL chunks (sc1 loads, its own included) and merges them in a fixed order —
// the output does not depend on the order of arrival — stores, and resets the ticket.
//
// Staging: K/V arrive by LDS-DMA into a two-buffer ring, the prefill kernel's path, not straight
// to VGPRs. The V^T operand of the second MFMA needs eight keys of one d per lane; from the
// row-major cache that is eight 2-byte loads per fragment, where LDS has the transposed read
// (ds_read_b64_tr_b16). With up to 64 query columns per K/V byte the MFMA form is kept for every
// T, and the DMA keeps a whole stage in flight per CU without holding VGPRs, of which the
// NG = 4, D = 128 instances need the most (resource remarks: profiles/decode/, profiles/decode_fp8/).
// DMA rows are clamped to the chunk's last valid key and DMA instructions of a wave tile that
// holds no valid key are skipped (ST = 2: every wait is vmcnt(0)), so stale cache rows past
// pos[b]+T, and their scales, are never read; keys past pos[b]+t are masked only on the wave
// tiles that hold one.
//
// Cache: the traits struct of a cache format. It states
//   Elem         the cache element type (its size gives the row bytes and the DMA source offsets),
//   SCALE_BYTES  bytes per key and operand of per-key fp32 scales staged next to a stage's rows
//                (0: none; else Operands holds Ks, Vs as [B][n_kv_head][C]),
//   Operands     the cache pointers; each(f) calls f with them in order. They are the kernel's
//                arguments kv_ptr, one restrict pointer each, so every instance keeps a plain argument
//                list (a longer or a differently laid out kernel-argument block costs step time),
//   operands(a)  those of a DecodeArgs (host),
// and does two things with the bytes in LDS, templates over the DecCfg:
//   k_frag(kb, row, ks, g)          the K fragment (A operand) of key `row`, elements 32ks + 8g .. +7,
//   pv(lo, hi, dx, ks, pf, o)       O^T += V^T P^T for one pair of transposed reads (32 row bytes).
#pragma once
#include <type_traits>

#include "attention_impl.h"

namespace dls_decode {

using dls_attn::BoolC;
using dls_attn::lds_bf16x4;
using dls_attn::raw_barrier;
using dls_attn::swz;
using dls_attn::wait_vm;
using dls_attn::xlane;

typedef __attribute__((address_space(3))) void lds_void;

constexpr int dec_waves(int D) { return D == 64 ? 4 : 2; }  // each takes 64 keys of a stage
// one chunk's published partial, field-major so that a wave's store or load of a field is one
// contiguous KB (write-through stores of part of a line are slow): o [NG][D/16][64 lanes] 16 B,
// then (m, l) [NG][64 lanes] 8 B. Which d a lane's o stands for is the format's; the bytes are not.
constexpr int ml_off(int D, int ng) { return ng * (D / 16) * 1024; }
constexpr int chunk_bytes(int D, int ng) { return ml_off(D, ng) + ng * 512; }

template <class Cache, int D, int NG_>
struct DecCfg {
  static constexpr int NG = NG_;                 // 16-wide query column groups
  static constexpr int KS = dec_waves(D);
  static constexpr int KT = 64;
  static constexpr int KTS = KT * KS;            // keys per stage (attn_decode_chunk)
  static constexpr int EB = sizeof(typename Cache::Elem);
  static constexpr int RB = D * EB;              // bytes per K/V row
  static constexpr int CH = RB / 16;             // 16-B chunks per row
  static constexpr int NVT = RB / 32;            // pairs of transposed V reads per row
  static constexpr int DI = D / 16 / NVT;        // d per 16-bit element of a V row, accumulated interleaved
  static constexpr int ROWS_PER_INSTR = 1024 / RB;
  static constexpr int INSTR = KTS / ROWS_PER_INSTR;  // per operand per stage
  static constexpr int PW = 2 * INSTR / KS;           // per wave per stage (K and V)
  static constexpr int TILE_BYTES = KTS * RB;
  static constexpr bool SCALED = Cache::SCALE_BYTES > 0;
  static constexpr int KSC_OFF = 2 * TILE_BYTES;      // K scales [KTS], then V scales
  static constexpr int VSC_OFF = KSC_OFF + KTS * Cache::SCALE_BYTES;
  static constexpr int BUF_BYTES = VSC_OFF + KTS * Cache::SCALE_BYTES;
  static constexpr int NQK = D / 32;
  static constexpr int ND = D / 16;
  static constexpr int REC = ND * 4 + 2;   // wave merge, floats per lane and group: o, m, l
  static constexpr int MERGE_BYTES = (KS - 1) * NG * 64 * REC * 4;
  static constexpr int SMEM = 2 * BUF_BYTES > MERGE_BYTES ? 2 * BUF_BYTES : MERGE_BYTES;
  static constexpr int ML_OFF = ml_off(D, NG);
  static constexpr int CHUNK_BYTES = chunk_bytes(D, NG);
  static_assert(PW * KS == 2 * INSTR && INSTR % PW == 0 && DI <= 2, "DMA split");
  static_assert(SMEM <= 163840, "LDS budget");
};

template <class Cache, int D, int NG, class... P>
__global__ __launch_bounds__(64 * dec_waves(D)) void attn_decode_kernel(
    const bf16* __restrict__ Q, int ldq, P* __restrict__... kv_ptr, bf16* __restrict__ O, int ldo,
    const int* __restrict__ pos, int T, int C, int KC, int n_head, int n_kv_head, float scale_log2,
    float* __restrict__ part, int* __restrict__ cnt) {
  using Cf = DecCfg<Cache, D, NG>;
  const typename Cache::Operands kv{kv_ptr...};
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

  // LDS-DMA: instruction j of this wave covers rows r0 .. r0+ROWS_PER_INSTR-1 of operand op (a
  // wave's instructions all belong to one operand). Sources are worked out per instruction, not
  // kept: PW pointers would cost the D = 128 instances 64 VGPRs. A scaled cache then fetches the
  // scales of the wave's own 64 keys, one fp32 per lane, with the rows' skip and the rows' clamp:
  // a scale of a key that is not valid never reaches arithmetic.
  const size_t ld = (size_t)n_kv_head * D;
  const int dop = hg * Cf::PW / Cf::INSTR;  // 0 = K, 1 = V
  const typename Cache::Elem* dbase = (dop == 0 ? kv.K : kv.V) + (size_t)b * C * ld + kvh * D;
  [[maybe_unused]] const size_t sbase = ((size_t)b * n_kv_head + kvh) * C;
  const int lrow = lane / Cf::CH, lch = lane % Cf::CH;
  auto issue = [&](int t) {
    char* buf = smem + (t & 1) * Cf::BUF_BYTES;
    // the operand's tile is formed here for an unscaled cache and at each instruction for a scaled
    // one: the compiler keeps the form it is given, and these are the ones each was measured with
    [[maybe_unused]] char* tile = buf + dop * Cf::TILE_BYTES;
    const int key0 = k_lo + t * Cf::KTS;
#pragma unroll
    for (int j = 0; j < Cf::PW; ++j) {
      const int r0 = ((hg * Cf::PW + j) % Cf::INSTR) * Cf::ROWS_PER_INSTR;
      if (key0 + r0 / Cf::KT * Cf::KT >= k_hi) continue;  // wave-uniform: that wave tile is not computed
      const int row = r0 + lrow;
      const int gch = lch ^ swz(row, Cf::CH - 1);
      const typename Cache::Elem* src = dbase + (size_t)min(key0 + row, k_hi - 1) * ld + gch * (16 / Cf::EB);
      char* dst = (Cf::SCALED ? buf + dop * Cf::TILE_BYTES : tile) + r0 * Cf::RB;
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)dst, 16, 0, 0);
    }
    if constexpr (Cf::SCALED) {
      if (key0 + hg * Cf::KT < k_hi) {  // wave-uniform
        const size_t si = sbase + min(key0 + hg * Cf::KT + lane, k_hi - 1);
        __builtin_amdgcn_global_load_lds((const void*)(kv.Ks + si), (lds_void*)(buf + Cf::KSC_OFF + hg * Cf::KT * 4),
                                         4, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(kv.Vs + si), (lds_void*)(buf + Cf::VSC_OFF + hg * Cf::KT * 4),
                                         4, 0, 0);
      }
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

  // which d of column ng*16 + li the element o[ng][x][i] stands for is the format's (pv, store)
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
        const bf16x8 kf = Cache::template k_frag<Cf>(kb, row, ks, g);
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) s[ng][n] = mfma16x16x32(kf, qf[ng][ks], s[ng][n]);
      }
    }
    // scores s[ng][n][i] <-> key key0 + 16n + 4g + i of column ng*16 + li. The scales of those
    // keys are applied in the swapped-operand form, not while converting: a key is a row of S^T,
    // so its K scale multiplies its fp32 score, and its V scale multiplies p before p is rounded to
    // bf16 — the SAME sixteen keys per lane, so a tile reads its scales as eight 16-byte LDS reads.
    [[maybe_unused]] f32x4 ksc[4], vsc[4];
    if constexpr (Cf::SCALED) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        ksc[n] = *reinterpret_cast<const f32x4*>(buf + Cf::KSC_OFF + (hg * Cf::KT + 16 * n + 4 * g) * 4);
        vsc[n] = *reinterpret_cast<const f32x4*>(buf + Cf::VSC_OFF + (hg * Cf::KT + 16 * n + 4 * g) * 4);
      }
    }
    bf16x8 pf[NG][2];
#pragma unroll
    for (int ng = 0; ng < NG; ++ng) {
      if constexpr (Cf::SCALED) {
#pragma unroll
        for (int n = 0; n < 4; ++n) s[ng][n] *= ksc[n];
      }
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
          float p = e;
          if constexpr (Cf::SCALED) p *= vsc[n][i];  // a masked key: 0 * a valid key's scale
          pf[ng][n >> 1][4 * (n & 1) + i] = f2bf(p);
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
    // element li of those 32 bytes from rows 32ks (+16) + 4g + 0..3.
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
        Cache::template pv<Cf>(lo, hi, dx, ks, pf, o);
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

  // merge the KS wave chains in one LDS exchange (field-major slabs, as attention_impl.h); wave 0
  // holds the result
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

  // wave 0: 32 row bytes of V hold M = 1 or 2 d per 16-bit element, accumulated d-interleaved in
  // o[ng][M*dx + q] (Cache::pv), so lane (g, li) has the 4M consecutive d = 16M*dx + 4M*g + M*i + q of
  // row O[b*T + t][(kvh*rep + r)*D ..] of column j = r*T + t = ng*16 + li
  auto store = [&](int ng, int dx, const f32x4& acc0, const f32x4& acc1, float l) {  // q = 0, q = M - 1
    constexpr int M = Cf::DI;
    const int j = ng * 16 + li;
    if (j >= ncol) return;
    const int r = j / T, t = j - r * T;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    std::conditional_t<M == 1, bf16x4, bf16x8> v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[M * i] = f2bf(acc0[i] * inv);
      if constexpr (M == 2) v[M * i + 1] = f2bf(acc1[i] * inv);
    }
    *reinterpret_cast<decltype(v)*>(O + ((size_t)b * T + t) * ldo + (kvh * rep + r) * D + 16 * M * dx + 4 * M * g) = v;
  };

  if (nact == 1) {
    if (hg != 0) return;
#pragma unroll
    for (int ng = 0; ng < NG; ++ng)
#pragma unroll
      for (int dx = 0; dx < Cf::NVT; ++dx) store(ng, dx, o[ng][Cf::DI * dx], o[ng][Cf::DI * dx + Cf::DI - 1], l_run[ng]);
    return;
  }

  // publish this chunk's (o, m, l)
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
  // the last arriver merges every chunk, its own included (sc1 loads: no stale copy): wave hg
  // takes chunks hg, hg + KS, ... in chunk order, all their fields in flight at once (one wave
  // walking every chunk field by field was a chain of dependent cross-XCD round trips that cost
  // more than the K/V stream), then the waves merge as above. Which chunk goes where is fixed,
  // so the sum does not depend on the order of arrival.
#pragma unroll
  for (int ng = 0; ng < NG; ++ng) {
    m_run[ng] = -INFINITY;
    l_run[ng] = 0.f;
#pragma unroll
    for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // U chunks' loads in flight together (a chunk past the last is read as the last and weighs
  // nothing); two at NG = 4, D = 128 would spill 44 bytes per lane to scratch
  constexpr int U = NG == 1 ? 4 : NG == 2 ? 2 : 1;
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
    for (int dx = 0; dx < Cf::NVT; ++dx) store(ng, dx, o[ng][Cf::DI * dx], o[ng][Cf::DI * dx + Cf::DI - 1], l_run[ng]);
}

// host side
inline int col_groups(const DecodeArgs& a) { return (a.n_head / a.n_kv_head * a.T + 15) / 16; }
inline int chunk_of(const DecodeArgs& a) {
  return a.chunk > 0 ? a.chunk : attn_decode_chunk(a.B, a.C, a.n_kv_head, a.D);
}

template <class Cache, int D, int NG>
void launch_decode(const DecodeArgs& a, int KC, hipStream_t s) {
  dim3 grid((a.C + KC - 1) / KC, a.n_kv_head, a.B), block(64 * dec_waves(D));
  Cache::operands(a).each([&](auto... p) {
    hipLaunchKernelGGL((attn_decode_kernel<Cache, D, NG, std::remove_pointer_t<decltype(p)>...>), grid, block, 0, s,
                       static_cast<const bf16*>(a.q), a.ldq, p..., static_cast<bf16*>(a.o), a.ldo, a.pos, a.T, a.C, KC,
                       a.n_head, a.n_kv_head, a.scale * 1.4426950408889634f, static_cast<float*>(a.part),
                       static_cast<int*>(a.cnt));
  });
}

template <class Cache, int D>
void launch_decode_d(const DecodeArgs& a, int ng, int KC, hipStream_t s) {
  switch (ng) {
    case 1: launch_decode<Cache, D, 1>(a, KC, s); break;
    case 2: launch_decode<Cache, D, 2>(a, KC, s); break;
    case 3: launch_decode<Cache, D, 3>(a, KC, s); break;
    default: launch_decode<Cache, D, 4>(a, KC, s); break;
  }
}

template <class Cache>
void launch_decode_any(const DecodeArgs& a, hipStream_t s) {
  const int KC = chunk_of(a), ng = col_groups(a);
  if (a.D == 64) launch_decode_d<Cache, 64>(a, ng, KC, s);
  else launch_decode_d<Cache, 128>(a, ng, KC, s);
}

}  // namespace dls_decode
