// Token sampling on the device: the launch that turns a decode step's logits into its next token.
//
// Grid (slices, B), 1024 threads. Row b*T + T-1 of the logits is split into `slices` contiguous
// runs of slice_len elements (a multiple of 8: every load is 16 bytes, the tail past V is masked
// by index, pad columns and other rows are never read).
//
// Phase 1, every slice: the largest order-preserving 16-bit key of the bf16 bits with its lowest
// index, and for sampling rows a histogram of the keys' high bytes (integer LDS atomics). With
// more than one slice the workgroup publishes both write-through (sc1), draws an agent-scope
// ticket of its row, and the last arriver reloads all slices (sc1 loads, its own included) and
// merges them: the pattern of attn_decode.hip; the last arriver resets the ticket, so the
// workspace needs zeroing once. Greedy rows end here: one pass over the logits.
//
// Phase 2, the last arriver alone, the row now in L2 / the Infinity Cache: top-k by two 8-bit
// radix levels of integer counts (level 1 came merged from the slices), top-p by two levels of
// per-bin weight sums, then the draw: per (tile, wave) sums in index order, the segment that
// crosses u*Z, the lane and the element inside it. That is up to four passes over the row by one
// CU, and its vector ALU is what they cost (about 15 us each at 128 256 logits; holding the row in
// registers across the passes, which was tried, changed nothing). So where top-k leaves at most
// 1024 entries (their number is known exactly from the counts) one pass collects them (index, key,
// weight) in LDS, and top-p and the draw are sums over that list, every thread over all of it:
// the same integers summed in another order, so the same theta, token and statistics as the
// passes would give.
//
// Determinism: weights are fixed-point integers, w_fx = rn(exp((l - l_max)/tau) * 2^40), summed
// in 64 bits (V <= 2^20 of them stay below 2^61), so every histogram bin, Z and every cumulative
// sum are exact integer sums that do not depend on the order of lanes, waves or workgroups;
// the comparison with u*Z, u = m * 2^-24, is the 128-bit integer comparison cum * 2^24 > m * Z.
// Since the kept weights sum to Z exactly and m < 2^24, some kept index always exceeds u*Z: the
// "largest kept index" fall-back of a floating-point sampler has no case here.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kThreads * 8;          // elements per pass iteration
constexpr int kWaveElems = 64 * 8;           // a wave's contiguous run inside a tile
constexpr int kPartWords = 264;              // per slice: 256 counts, key:index of the max, pad to 16 B
constexpr int kMaxSeg = kSampleMaxV / kTile * kWaves;
constexpr float kFxScale = 1099511627776.f;  // 2^40
constexpr float kFxInv = 1.f / 1099511627776.f;
constexpr uint32_t kKeyNegInf = 0x007fu;
constexpr int kListCap = 1024;               // top-k survivors up to this many are finished from a list in LDS

// bf16 bits -> 16-bit key whose unsigned order is the order of the values (-0 counts as +0)
__device__ __forceinline__ uint32_t key_of(uint32_t bits) {
  if (bits == 0x8000u) bits = 0;
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}
__device__ __forceinline__ float val_of(uint32_t key) {
  const uint32_t bits = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(bits << 16);
}
__device__ __forceinline__ uint32_t key_at(const u32x4& v, int i) {
  const uint32_t w = v[i >> 1];
  return key_of((i & 1) ? (w >> 16) : (w & 0xffffu));
}
__device__ __forceinline__ u64 weight_fx(uint32_t key, float lmax, float tau) {
  const float w = __expf((val_of(key) - lmax) / tau);  // -inf -> 0
  return (u64)__float2ull_rn(w * kFxScale);
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
  return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, shfl_xor64(v, o));
  return v;
}
__device__ __forceinline__ u64 wave_incl_scan64(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = shfl_up64(v, o);
    if (lane >= o) v += y;
  }
  return v;
}

// cum * 2^24 > m * Z in 128 bits (cum < 2^61, m < 2^24)
__device__ __forceinline__ bool exceeds(u64 cum, u64 m, u64 Z) {
  const u64 lhi = cum >> 40, llo = cum << 24;
  const u64 rhi = __umul64hi(m, Z), rlo = m * Z;
  return lhi > rhi || (lhi == rhi && llo > rlo);
}

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return __umulhi(a, b); }

// Philox4x32-10, word 0 of the output
__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return c0;
}

// Wave 0: the first of the 256 bins, walking from bin 255 down, at which base + (sum of the bins
// walked) reaches the target; out[0] = bin, out[1] = the sum before it, out[2] = the target. With
// frac < 1 the target is ceil(frac * (base + sum of all bins)), else `target`.
template <typename T>
__device__ __forceinline__ void find_desc(const T* hist, u64 base, u64 target, float frac, int lane, u64* out) {
  u64 v[4], local = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = hist[255 - 4 * lane - j];
    local += v[j];
  }
  const u64 incl = wave_incl_scan64(local, lane);
  if (frac < 1.f) {
    const u64 total = base + shfl64(incl, 63);
    const double t = ceil((double)frac * (double)total);
    target = min(max((u64)t, (u64)1), total);
  }
  u64 c = base + incl - local;
  int bin = -1;
  u64 before = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (bin < 0 && c + v[j] >= target) bin = 255 - 4 * lane - j, before = c;
    c += v[j];
  }
  const u64 hit = __ballot(bin >= 0);
  const int first = hit ? __ffsll((long long)hit) - 1 : 0;
  if (lane == first) out[0] = bin < 0 ? 0 : bin, out[1] = before, out[2] = target;
}

__global__ __launch_bounds__(kThreads) void sample_kernel(SampleArgs a, int S, int slice_len) {
  __shared__ u64 hw[256];
  __shared__ u64 seg[kMaxSeg];
  __shared__ u64 red[kWaves];
  __shared__ u64 bc[4];
  __shared__ uint32_t hc[256];
  __shared__ int flag;
  __shared__ uint32_t lcount, lth;
  const int s = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const bf16* row = static_cast<const bf16*>(a.logits) + ((size_t)b * a.T + a.T - 1) * a.ld;
  const float tau = a.temperature[b];
  const bool greedy = !(tau > 0.f);

  // ---- phase 1: this slice's maximum (lowest index on ties) and level-1 counts
  if (tid < 256) hc[tid] = 0;
  __syncthreads();
  const int lo = s * slice_len, hi = min(lo + slice_len, V);
  u64 best = 0;  // key << 32 | ~index: the largest is the largest key at its lowest index
  for (int base = lo + tid * 8; base < hi; base += kTile) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + base);
    const int nv = hi - base;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nv) {
        const uint32_t key = key_at(v, i);
        best = max(best, ((u64)key << 32) | (0xffffffffu - (uint32_t)(base + i)));
        if (!greedy) atomicAdd(&hc[key >> 8], 1u);
      }
    }
  }
  best = wave_max64(best);
  if (lane == 0) red[wave] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) best = max(best, red[w]);

  if (S > 1) {
    // publish (write-through), ticket, and the last arriver merges every slice in slice order
    const auto rp = __builtin_amdgcn_make_buffer_rsrc(a.part + (size_t)b * S * kPartWords, 0, 0x7fffffff, 0x00020000);
    if (!greedy && tid < 64)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{hc[4 * tid], hc[4 * tid + 1], hc[4 * tid + 2], hc[4 * tid + 3]}, rp,
                                             (s * kPartWords + 4 * tid) * 4, 0, 16);
    if (tid == 0)
      __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)(best >> 32), (uint32_t)best}, rp,
                                            (s * kPartWords + 256) * 4, 0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-through stores landed
    __syncthreads();
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(a.cnt + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == S - 1;
      if (last) __hip_atomic_store(a.cnt + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
      flag = last;
    }
    __syncthreads();
    if (!flag) return;  // block-uniform
    if (!greedy && tid < 256) {
      uint32_t c = 0;
      for (int s2 = 0; s2 < S; ++s2) c += __builtin_amdgcn_raw_buffer_load_b32(rp, (s2 * kPartWords + tid) * 4, 0, 16);
      hc[tid] = c;
    }
    if (wave == 0) {
      u64 bb = 0;
      for (int s2 = lane; s2 < S; s2 += 64) {
        const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(rp, (s2 * kPartWords + 256) * 4, 0, 16);
        bb = max(bb, ((u64)x[0] << 32) | x[1]);
      }
      bb = wave_max64(bb);
      if (lane == 0) bc[0] = bb;
    }
    __syncthreads();
    best = bc[0];
  }

  const uint32_t kmax = (uint32_t)(best >> 32);
  const float lmax = val_of(kmax);

  // the stream rule; one lane of the workgroup calls it
  auto finish = [&](int token, float theta, float Z, float before, float wtok) {
    const int n = a.pos[b] + a.T;
    const int pl = a.prompt_len ? a.prompt_len[b] : 0;
    const int eos = a.eos ? a.eos[0] : -1;
    int next = token;
    if (n < pl) {
      if (n >= 0 && n < a.C) next = a.tokens[(size_t)b * a.C + n];  // the prompt is forced
    } else {
      if (a.done && a.done[b]) next = eos;
      if (a.done && eos >= 0 && next == eos) a.done[b] = 1;
      if (n >= 0 && n < a.C) a.tokens[(size_t)b * a.C + n] = next;
    }
    a.next_out[b] = next;
    *reinterpret_cast<f32x4*>(a.stats + (size_t)b * 4) = f32x4{theta, Z, before, wtok};
  };

  if (greedy) {
    if (tid == 0) finish((int)(0xffffffffu - (uint32_t)best), lmax, 1.f, 0.f, 1.f);
    return;
  }

  // ---- phase 2 (one workgroup per row)
  // a pass over the whole row: f(key) for every valid element
  auto pass = [&](auto f) {
    for (int base = tid * 8; base < V; base += kTile) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(row + base);
      const int nv = V - base;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < nv) f(key_at(v, i));
    }
  };
  // wave 0 walks a finished histogram; everyone gets (bin, sum before it, target)
  auto pick = [&](auto* hist, u64 base, u64 target, float frac, u64& before, u64& tgt) -> uint32_t {
    __syncthreads();
    if (wave == 0) find_desc(hist, base, target, frac, lane, bc);
    __syncthreads();
    const uint32_t bin = (uint32_t)bc[0];
    before = bc[1], tgt = bc[2];
    __syncthreads();
    return bin;
  };

  const int k = a.top_k[b];
  const float p = a.top_p[b];
  uint32_t kth = kKeyNegInf;
  int kept_n = V;  // entries >= theta_k
  if (k > 0 && k < V) {  // theta_k: the k-th largest, by counts
    u64 above, above2, tg;
    const uint32_t hb = pick(hc, 0, (u64)k, 1.f, above, tg);
    if (tid < 256) hc[tid] = 0;
    __syncthreads();
    pass([&](uint32_t key) {
      if ((key >> 8) == hb) atomicAdd(&hc[key & 255u], 1u);
    });
    const uint32_t lb = pick(hc, above, (u64)k, 1.f, above2, tg);
    kth = (hb << 8) | lb;
    kept_n = (int)(above2 + hc[lb]);
  }
  const int n = a.pos[b] + a.T;
  const long long seed = a.seed[0];
  const u64 m = philox_x0((uint32_t)n, (uint32_t)b, (uint32_t)a.request, 0u, (uint32_t)seed,
                          (uint32_t)((u64)seed >> 32)) >> 8;

  if (kept_n <= kListCap) {  // block-uniform
    u64* lw = seg;  // the list lives where the long path keeps its segment sums
    uint32_t* lidx = reinterpret_cast<uint32_t*>(seg + kListCap);
    uint32_t* lkey = lidx + kListCap;
    if (tid == 0) lcount = 0, lth = 0;
    __syncthreads();
    for (int base = tid * 8; base < V; base += kTile) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(row + base);
      const int nv = V - base;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t key = key_at(v, i);
        if (i < nv && key >= kth) {
          const uint32_t slot = atomicAdd(&lcount, 1u);
          if (slot < (uint32_t)kListCap) lidx[slot] = base + i, lkey[slot] = key, lw[slot] = weight_fx(key, lmax, tau);
        }
      }
    }
    __syncthreads();
    const int nl = min((int)lcount, kListCap);  // == kept_n
    const bool mine = tid < nl;
    const uint32_t mykey = mine ? lkey[tid] : 0u, myidx = mine ? lidx[tid] : 0u;
    const u64 myw = mine ? lw[tid] : 0;
    uint32_t th = kth;
    if (p < 1.f) {  // the largest value whose classes, with all above them, weigh p * Z1
      u64 incl = 0, total = 0;
      for (int j = 0; j < nl; ++j) {
        const u64 wj = lw[j];
        total += wj;
        if (lkey[j] >= mykey) incl += wj;
      }
      const double t = ceil((double)p * (double)total);
      const u64 target = min(max((u64)t, (u64)1), total);
      if (mine && incl >= target) atomicMax(&lth, mykey);
      __syncthreads();
      th = lth;
    }
    u64 before = 0, Z = 0;
    for (int j = 0; j < nl; ++j) {
      const u64 wj = lkey[j] >= th ? lw[j] : 0;
      Z += wj;
      if (lidx[j] < myidx) before += wj;
    }
    // one entry's interval holds u * Z: the cumulative sums rise to Z and a weightless entry's is empty
    if (mine && mykey >= th && !exceeds(before, m, Z) && exceeds(before + myw, m, Z))
      finish((int)myidx, val_of(th), (float)Z * kFxInv, (float)before * kFxInv, (float)myw * kFxInv);
    return;
  }

  uint32_t th = kth;
  if (p < 1.f) {  // theta: the first value, walking down, whose classes weigh p * Z1
    if (tid < 256) hw[tid] = 0;
    __syncthreads();
    pass([&](uint32_t key) {
      if (key >= kth) {
        const u64 w = weight_fx(key, lmax, tau);
        if (w) atomicAdd(&hw[key >> 8], w);
      }
    });
    u64 above, tg;
    const uint32_t hb = pick(hw, 0, 0, p, above, tg);
    if (tid < 256) hw[tid] = 0;
    __syncthreads();
    pass([&](uint32_t key) {
      if (key >= kth && (key >> 8) == hb) {
        const u64 w = weight_fx(key, lmax, tau);
        if (w) atomicAdd(&hw[key & 255u], w);
      }
    });
    u64 tg2;
    th = (hb << 8) | pick(hw, above, tg, 1.f, above, tg2);
  }

  // ---- the draw: sums of the kept weights per (tile, wave), which is index order
  const int ntile = (V + kTile - 1) / kTile;
  auto tile_sum = [&](const u32x4& v, int j) {
    const int nv = V - (j * kTile + tid * 8);
    u64 sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t key = key_at(v, i);
      if (i < nv && key >= th) sum += weight_fx(key, lmax, tau);
    }
    sum = wave_sum64(sum);
    if (lane == 0) seg[j * kWaves + wave] = sum;
  };
  for (int j = 0; j < ntile; ++j) {
    const int base = j * kTile + tid * 8;
    tile_sum(base < V ? *reinterpret_cast<const u32x4*>(row + base) : u32x4{0u, 0u, 0u, 0u}, j);
  }
  __syncthreads();
  if (wave != 0) return;
  const int nseg = ntile * kWaves;
  u64 Z = 0;
  for (int i = lane; i < nseg; i += 64) Z += seg[i];
  Z = wave_sum64(Z);
  // the segment whose inclusive sum first exceeds u * Z
  int sidx = nseg - 1;
  u64 before = 0, run = 0;
  for (int c0 = 0; c0 < nseg; c0 += 64) {
    const u64 v = c0 + lane < nseg ? seg[c0 + lane] : 0;
    const u64 incl = run + wave_incl_scan64(v, lane);
    const u64 hit = __ballot(exceeds(incl, m, Z));
    if (hit) {
      const int first = __ffsll((long long)hit) - 1;
      sidx = c0 + first;
      before = shfl64(incl - v, first);
      break;
    }
    run = shfl64(incl, 63);
  }
  // inside it: the lane, then the element
  const int base = (sidx / kWaves) * kTile + (sidx % kWaves) * kWaveElems + lane * 8;
  u64 w[8], lsum = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0;
  bool kept[8] = {};
  if (base < V) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + base);
    const int nv = V - base;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t key = key_at(v, i);
      kept[i] = i < nv && key >= th;
      if (kept[i]) w[i] = weight_fx(key, lmax, tau), lsum += w[i];
    }
  }
  const u64 incl = before + wave_incl_scan64(lsum, lane);
  const u64 hit = __ballot(exceeds(incl, m, Z));
  const int first = hit ? __ffsll((long long)hit) - 1 : 0;
  if (lane != first) return;
  u64 c = incl - lsum;
  int token = base;
  u64 cb = c, wt = 0;
  bool found = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!found && kept[i] && exceeds(c + w[i], m, Z)) found = true, token = base + i, cb = c, wt = w[i];
    c += w[i];
  }
  finish(token, val_of(th), (float)Z * kFxInv, (float)cb * kFxInv, (float)wt * kFxInv);
}

}  // namespace

void sample_slices(int B, int V, int* slices, int* slice_len) {
  // a slice is at least one pass of a workgroup (8192 elements); at most 64 slices a row, and
  // no more workgroups than two rounds of the chip
  int S = std::min(64, (V + kTile - 1) / kTile);
  S = std::max(1, std::min(S, 512 / std::max(B, 1)));
  const int v8 = (V + 7) / 8;
  const int len = (v8 + S - 1) / S * 8;
  *slice_len = len;
  *slices = (V + len - 1) / len;  // no empty slice
}

void sample_sizes(int B, int V, size_t* part_words, size_t* counters) {
  int S, len;
  sample_slices(B, V, &S, &len);
  *part_words = (size_t)B * S * kPartWords;
  *counters = (size_t)B;
}

void launch_sample(const SampleArgs& a, hipStream_t s) {
  int S, len;
  sample_slices(a.B, a.V, &S, &len);
  hipLaunchKernelGGL(sample_kernel, dim3(S, a.B), dim3(kThreads), 0, s, a, S, len);
}
