// KV cache and decode attention on MFMA, bf16 caches — the step that extends every sequence by
// T <= 16 tokens against keys it already holds.
//
// attn_decode: workgroup = one (key chunk of KC keys, KV head, sequence). Its query rows are the
// rep*T rows of the KV head's rep = n_head/n_kv_head query heads, packed as the 16-wide operand
// columns of the swapped-operand formulation of attention_impl.h (S^T = K Q^T, O^T += V^T P^T;
// column j = r*T + t is new token t of query head kvh*rep + r), NG = ceil(rep*T/16) column groups
// per wave: every K and V fragment is read from LDS once and used by NG MFMAs, so the K/V bytes
// are read once per KV head, not once per query head. The KS waves of the workgroup each walk
// 64 of a stage's keys with an online-softmax chain of their own and are merged through LDS.
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
// T, and the DMA keeps a whole stage (64 KB) in flight per CU without holding VGPRs, of which the
// NG = 4, D = 128 instance needs the most (resource remarks: profiles/decode/).
// DMA rows are clamped to the chunk's last valid key and DMA instructions of a wave tile that
// holds no valid key are skipped (ST = 2: every wait is vmcnt(0)), so stale cache rows past
// pos[b]+T are never read; keys past pos[b]+t are masked only on the wave tiles that hold one.
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

template <int D, int NG_>
struct DecCfg {
  static constexpr int NG = NG_;                 // 16-wide query column groups
  static constexpr int KS = D == 64 ? 4 : 2;     // waves: each takes 64 keys of a stage
  static constexpr int KT = 64;
  static constexpr int KTS = KT * KS;            // keys per stage
  static constexpr int RB = D * 2;               // bytes per K/V row
  static constexpr int CH = D / 8;               // 16-B chunks per row
  static constexpr int ROWS_PER_INSTR = 1024 / RB;
  static constexpr int INSTR = KTS / ROWS_PER_INSTR;  // per operand per stage
  static constexpr int PW = 2 * INSTR / KS;           // per wave per stage (K and V)
  static constexpr int TILE_BYTES = KTS * RB;
  static constexpr int BUF_BYTES = 2 * TILE_BYTES;
  static constexpr int NQK = D / 32;
  static constexpr int ND = D / 16;
  static constexpr int REC = ND * 4 + 2;   // wave merge, floats per lane and group: o, m, l
  static constexpr int MERGE_BYTES = (KS - 1) * NG * 64 * REC * 4;
  static constexpr int SMEM = 2 * BUF_BYTES > MERGE_BYTES ? 2 * BUF_BYTES : MERGE_BYTES;
  // one chunk's published partial, field-major so that a wave's store or load of a field is one
  // contiguous KB (write-through stores of part of a line are slow): o [NG][ND][64 lanes] 16 B,
  // then (m, l) [NG][64 lanes] 8 B
  static constexpr int ML_OFF = NG * ND * 1024;
  static constexpr int CHUNK_BYTES = ML_OFF + NG * 512;
  static_assert(PW * KS == 2 * INSTR && INSTR % PW == 0, "DMA split");
  static_assert(SMEM <= 163840, "LDS budget");
};

template <int D>
constexpr int kDecThreads = 64 * DecCfg<D, 1>::KS;

template <int D, int NG>
__global__ __launch_bounds__(kDecThreads<D>) void attn_decode_kernel(
    const bf16* __restrict__ Q, int ldq, const bf16* __restrict__ Kc, const bf16* __restrict__ Vc,
    bf16* __restrict__ O, int ldo, const int* __restrict__ pos, int T, int C, int KC, int n_head, int n_kv_head,
    float scale_log2, float* __restrict__ part, int* __restrict__ cnt) {
  using Cf = DecCfg<D, NG>;
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
  // kept: PW pointers would cost the D = 128 instances 64 VGPRs.
  const size_t ld = (size_t)n_kv_head * D;
  const int dop = hg * Cf::PW / Cf::INSTR;  // 0 = K, 1 = V
  const bf16* dbase = (dop == 0 ? Kc : Vc) + (size_t)b * C * ld + kvh * D;
  const int lrow = lane / Cf::CH, lch = lane % Cf::CH;
  auto issue = [&](int t) {
    char* buf = smem + (t & 1) * Cf::BUF_BYTES + dop * Cf::TILE_BYTES;
    const int key0 = k_lo + t * Cf::KTS;
#pragma unroll
    for (int j = 0; j < Cf::PW; ++j) {
      const int r0 = ((hg * Cf::PW + j) % Cf::INSTR) * Cf::ROWS_PER_INSTR;
      if (key0 + r0 / Cf::KT * Cf::KT >= k_hi) continue;  // wave-uniform: that wave tile is not computed
      const int row = r0 + lrow;
      const int gch = lch ^ swz(row, Cf::CH - 1);
      const bf16* src = dbase + (size_t)min(key0 + row, k_hi - 1) * ld + gch * 8;
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(buf + r0 * Cf::RB), 16, 0, 0);
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
    const char* kb = smem + (t & 1) * Cf::BUF_BYTES + hg * Cf::KT * Cf::RB;
    const char* vb = kb + Cf::TILE_BYTES;
    f32x4 s[NG][4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int ng = 0; ng < NG; ++ng) s[ng][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int row = 16 * n + li;
#pragma unroll
      for (int ks = 0; ks < Cf::NQK; ++ks) {
        const int ch = 4 * ks + g;
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + row * Cf::RB + ((ch ^ swz(row, Cf::CH - 1)) << 4));
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) s[ng][n] = mfma16x16x32(kf, qf[ng][ks], s[ng][n]);
      }
    }
    // scores s[ng][n][i] <-> key key0 + 16n + 4g + i of column ng*16 + li
    bf16x8 pf[NG][2];
#pragma unroll
    for (int ng = 0; ng < NG; ++ng) {
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
          pf[ng][n >> 1][4 * (n & 1) + i] = f2bf(e);
        }
      sum = xlane<false, 16>(sum);
      sum = xlane<false, 32>(sum);
      l_run[ng] = l_run[ng] * alpha + sum;
      m_run[ng] = m_new;
#pragma unroll
      for (int dn = 0; dn < Cf::ND; ++dn) o[ng][dn] *= alpha;
    }
    // O^T += V^T P^T ; V^T fragment element j <-> key 32ks + 16(j>>2) + 4g + (j&3)
    const int q4 = li >> 2, p4 = li & 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int dn = 0; dn < Cf::ND; ++dn) {
        const int ch = 2 * dn + (p4 >> 1);
        const int row0 = 32 * ks + 4 * g + q4;
        const int row1 = row0 + 16;
        const lds_bf16x4* a0 =
            (const lds_bf16x4*)(vb + row0 * Cf::RB + ((ch ^ swz(row0, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const lds_bf16x4* a1 =
            (const lds_bf16x4*)(vb + row1 * Cf::RB + ((ch ^ swz(row1, Cf::CH - 1)) << 4) + (p4 & 1) * 8);
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) o[ng][dn] = mfma16x16x32(vf, pf[ng][ks], o[ng][dn]);
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

  // O[b*T + t][(kvh*rep + r)*D + 16dn + 4g + i] of column j = r*T + t = ng*16 + li
  auto store = [&](int ng, int dn, const f32x4& acc, float l) {
    const int j = ng * 16 + li;
    if (j >= ncol) return;
    const int r = j / T, t = j - r * T;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    bf16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = f2bf(acc[i] * inv);
    *reinterpret_cast<bf16x4*>(O + ((size_t)b * T + t) * ldo + (kvh * rep + r) * D + 16 * dn + 4 * g) = v;
  };

  if (nact == 1) {
    if (hg != 0) return;
#pragma unroll
    for (int ng = 0; ng < NG; ++ng)
#pragma unroll
      for (int dn = 0; dn < Cf::ND; ++dn) store(ng, dn, o[ng][dn], l_run[ng]);
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
    for (int dn = 0; dn < Cf::ND; ++dn) store(ng, dn, o[ng][dn], l_run[ng]);
}

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

template <int D, int NG>
void launch_decode(const DecodeArgs& a, int KC, hipStream_t s) {
  using Cf = DecCfg<D, NG>;
  dim3 grid((a.C + KC - 1) / KC, a.n_kv_head, a.B), block(64 * Cf::KS);
  hipLaunchKernelGGL((attn_decode_kernel<D, NG>), grid, block, 0, s, static_cast<const bf16*>(a.q), a.ldq,
                     static_cast<const bf16*>(a.k_cache), static_cast<const bf16*>(a.v_cache),
                     static_cast<bf16*>(a.o), a.ldo, a.pos, a.T, a.C, KC, a.n_head, a.n_kv_head,
                     a.scale * 1.4426950408889634f, static_cast<float*>(a.part), static_cast<int*>(a.cnt));
}

template <int D>
void launch_decode_d(const DecodeArgs& a, int ng, int KC, hipStream_t s) {
  switch (ng) {
    case 1: launch_decode<D, 1>(a, KC, s); break;
    case 2: launch_decode<D, 2>(a, KC, s); break;
    case 3: launch_decode<D, 3>(a, KC, s); break;
    default: launch_decode<D, 4>(a, KC, s); break;
  }
}

int col_groups(const DecodeArgs& a) { return (a.n_head / a.n_kv_head * a.T + 15) / 16; }
int chunk_of(const DecodeArgs& a) { return a.chunk > 0 ? a.chunk : attn_decode_chunk(a.B, a.C, a.n_kv_head, a.D); }

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
  const int KC = chunk_of(a);
  const size_t maxc = (a.C + KC - 1) / KC;
  *counters = (size_t)a.B * a.n_kv_head;
  *part_floats = *counters * maxc * col_groups(a) * 64 * (a.D / 16 * 4 + 2);  // DecCfg::CHUNK_BYTES / 4
}

void launch_attn_decode(const DecodeArgs& a, hipStream_t s) {
  if (a.kv_fp8) return launch_attn_decode_fp8(a, s);  // attn_decode_fp8.hip
  const int KC = chunk_of(a), ng = col_groups(a);
  if (a.D == 64) launch_decode_d<64>(a, ng, KC, s);
  else launch_decode_d<128>(a, ng, KC, s);
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
