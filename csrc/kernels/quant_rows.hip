// Per-row e4m3 quantisation of bf16 activation rows, alone and fused behind a norm.
//
//   q[m][k] = rne(clamp(x[m][k] / scale[m], +-448)) as OCP e4m3, scale[m] fp32 = the smallest
//   power of two with amax_m / scale[m] <= 448 (an all-zero row: 1)
//
// — the semantics of models/params.py quantize_fp8, byte for byte: dividing by a power of two
// is exact (v_ldexp_f32), the clamp is done in software before v_cvt_pk_fp8_f32, and the
// conversion rounds to nearest even, subnormals included.
//
// quant_rows_kernel: WPR waves per row (1 for K <= 1024, up to 4), the row held in registers
// between the amax pass and the convert pass (16-B chunks, 8 bf16 per lane, MAXQ per lane);
// what a longer row has beyond that is read a second time (it comes from L2).
//
// norm_q8_kernel: the body of norm.hip's norm_kernel — the same loads, the same statistics in
// the same order, the same normalise expression — whose epilogue rounds the normalised value
// to bf16 (what the norm kernel would have stored), takes the row's amax of THOSE values and
// emits (q, scale) instead of bf16 rows: bitwise what quant_rows(norm(x)) gives, one launch
// and one HBM write of 1 byte per element instead of 2 + a second launch.
#include "common.h"
#include "kernels.h"

namespace {

// scale exponent e of quantize_fp8: amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
__device__ __forceinline__ int scale_exp(float amax) {
  int ex;
  const float m = frexpf(amax, &ex);
  return m <= 0.875f ? ex - 9 : ex - 8;
}

// 8 bf16-valued floats / 2^e -> 8 e4m3 bytes
__device__ __forceinline__ u32x2 quant8(const float* v, int e) {
  float t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = fminf(fmaxf(ldexpf(v[i], -e), -448.f), 448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}

constexpr int MAXQ = 8;  // 16-B chunks a lane keeps in registers

template <int WPR>
__global__ __launch_bounds__(256) void quant_rows_kernel(const bf16* __restrict__ x, int ldx,
                                                         uint8_t* __restrict__ q, int ldq,
                                                         float* __restrict__ scale, int M, int K) {
  constexpr int RPB = 4 / WPR;  // rows per 256-thread block
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = wave % WPR;
  const int row = blockIdx.x * RPB + wave / WPR;
  const bool active = row < M;
  const int nch = K / 8;
  const int stride = 64 * WPR;
  const int base = sub * 64 + lane;
  const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + (size_t)(active ? row : 0) * ldx);
  bf16x8 xa[MAXQ];
#pragma unroll
  for (int c = 0; c < MAXQ; ++c) {
    const int ch = base + c * stride;
    if (active && ch < nch) xa[c] = xr[ch];
  }
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < MAXQ; ++c) {
    const int ch = base + c * stride;
    if (active && ch < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(xa[c][e])));
    }
  }
  if (active)
    for (int ch = base + MAXQ * stride; ch < nch; ch += stride) {
      const bf16x8 a = xr[ch];
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(a[e])));
    }
  amax = wave_max(amax);
  if (WPR > 1) {
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    const int w0 = (wave / WPR) * WPR;
    amax = red[w0];
#pragma unroll
    for (int k = 1; k < WPR; ++k) amax = fmaxf(amax, red[w0 + k]);
  }
  if (!active) return;
  const int e = amax > 0.f ? scale_exp(amax) : 0;
  if (sub == 0 && lane == 0) scale[row] = ldexpf(1.0f, e);
  u32x2* qr = reinterpret_cast<u32x2*>(q + (size_t)row * ldq);
#pragma unroll
  for (int c = 0; c < MAXQ; ++c) {
    const int ch = base + c * stride;
    if (ch < nch) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = bf2f(xa[c][i]);
      qr[ch] = quant8(v, e);
    }
  }
  for (int ch = base + MAXQ * stride; ch < nch; ch += stride) {
    const bf16x8 a = xr[ch];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(a[i]);
    qr[ch] = quant8(v, e);
  }
}

constexpr int MAXC = 4;  // as norm.hip: H <= 8 * 64 * WPR * MAXC (8192 at WPR = 4)

template <bool RMS, int WPR>
__global__ __launch_bounds__(256) void norm_q8_kernel(const bf16* __restrict__ x, const bf16* __restrict__ r,
                                                      bf16* __restrict__ sum_out, const bf16* __restrict__ w,
                                                      const bf16* __restrict__ b, uint8_t* __restrict__ q,
                                                      float* __restrict__ scale, int M, int H, float eps) {
  constexpr int RPB = 4 / WPR;  // rows per 256-thread block
  __shared__ float red[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = wave % WPR;                 // this wave's slice of the row
  const int row = blockIdx.x * RPB + wave / WPR;
  const bool active = row < M;
  const int nch = H / 8;
  const int stride = 64 * WPR;
  const int base = sub * 64 + lane;
  const size_t roff = (size_t)(active ? row : 0) * H;
  const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + roff);
  const bf16x8* rr = r ? reinterpret_cast<const bf16x8*>(r + roff) : nullptr;
  const bf16x8* wr = reinterpret_cast<const bf16x8*>(w);
  const bf16x8* br = b ? reinterpret_cast<const bf16x8*>(b) : nullptr;
  bf16x8 xa[MAXC], ra[MAXC], wa[MAXC], ba[MAXC];
  // issue every load first
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = base + c * stride;
    if (active && ch < nch) {
      xa[c] = xr[ch];
      if (rr) ra[c] = rr[ch];
      wa[c] = wr[ch];
      if (br) ba[c] = br[ch];
    }
  }
  float v[MAXC][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = base + c * stride;
    if (active && ch < nch) {
      bf16x8 a = xa[c];
      if (rr) {
        bf16x8 sum;
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[e] = f2bf(bf2f(a[e]) + bf2f(ra[c][e]));
        a = sum;
        if (sum_out) reinterpret_cast<bf16x8*>(sum_out + roff)[ch] = sum;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[c][e] = bf2f(a[e]);
        s += RMS ? v[c][e] * v[c][e] : v[c][e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
    }
  }
  auto row_sum = [&](float t, int slot) {
    t = wave_sum(t);
    if (WPR == 1) return t;
    if (lane == 0) red[slot][wave] = t;
    __syncthreads();
    float tot = 0.f;
    const int w0 = (wave / WPR) * WPR;
#pragma unroll
    for (int k = 0; k < WPR; ++k) tot += red[slot][w0 + k];
    return tot;
  };
  s = row_sum(s, 0);
  float mean = 0.f, rstd;
  if (RMS) {
    rstd = rsqrtf(s / H + eps);
  } else {
    mean = s / H;
    float qq = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = base + c * stride;
      if (active && ch < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[c][e] - mean;
          qq += d * d;
        }
      }
    }
    qq = row_sum(qq, 1);
    rstd = rsqrtf(qq / H + eps);
  }
  // the normalised row, rounded to bf16 as the norm kernel stores it, and its amax
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = base + c * stride;
    if (active && ch < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float o = (v[c][e] - mean) * rstd * bf2f(wa[c][e]);
        if (br) o += bf2f(ba[c][e]);
        v[c][e] = bf2f(f2bf(o));
        amax = fmaxf(amax, fabsf(v[c][e]));
      }
    }
  }
  amax = wave_max(amax);
  if (WPR > 1) {
    if (lane == 0) red[2][wave] = amax;
    __syncthreads();
    const int w0 = (wave / WPR) * WPR;
    amax = red[2][w0];
#pragma unroll
    for (int k = 1; k < WPR; ++k) amax = fmaxf(amax, red[2][w0 + k]);
  }
  if (!active) return;
  const int e = amax > 0.f ? scale_exp(amax) : 0;
  if (sub == 0 && lane == 0) scale[row] = ldexpf(1.0f, e);
  u32x2* qr = reinterpret_cast<u32x2*>(q + roff);
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = base + c * stride;
    if (ch < nch) qr[ch] = quant8(v[c], e);
  }
}

template <bool RMS>
void launch_norm_q8_t(const void* x, const void* r, void* sum_out, const void* w, const void* b, void* q,
                      float* scale, int M, int H, float eps, hipStream_t s) {
  // waves per row: the rule of norm.hip
  const int nch = H / 8;
  int wpr = 1;
  while (wpr < 4 && (nch > 64 * wpr * MAXC || (H >= 2048 && wpr * 1024 < H))) wpr *= 2;
  const dim3 block(256);
  const auto* xp = (const bf16*)x;
  const auto* rp = (const bf16*)r;
  auto* sp = (bf16*)sum_out;
  const auto* wp = (const bf16*)w;
  const auto* bp = (const bf16*)b;
  auto* qp = (uint8_t*)q;
  if (wpr == 1)
    hipLaunchKernelGGL((norm_q8_kernel<RMS, 1>), dim3((M + 3) / 4), block, 0, s, xp, rp, sp, wp, bp, qp, scale, M,
                       H, eps);
  else if (wpr == 2)
    hipLaunchKernelGGL((norm_q8_kernel<RMS, 2>), dim3((M + 1) / 2), block, 0, s, xp, rp, sp, wp, bp, qp, scale, M,
                       H, eps);
  else
    hipLaunchKernelGGL((norm_q8_kernel<RMS, 4>), dim3(M), block, 0, s, xp, rp, sp, wp, bp, qp, scale, M, H, eps);
}

}  // namespace

void launch_quant_rows_fp8(const void* x, int ldx, void* q, int ldq, float* scale, int M, int K, hipStream_t s) {
  const auto* xp = (const bf16*)x;
  auto* qp = (uint8_t*)q;
  const dim3 block(256);
  if (K <= 1024)
    hipLaunchKernelGGL((quant_rows_kernel<1>), dim3((M + 3) / 4), block, 0, s, xp, ldx, qp, ldq, scale, M, K);
  else if (K <= 2048)
    hipLaunchKernelGGL((quant_rows_kernel<2>), dim3((M + 1) / 2), block, 0, s, xp, ldx, qp, ldq, scale, M, K);
  else
    hipLaunchKernelGGL((quant_rows_kernel<4>), dim3(M), block, 0, s, xp, ldx, qp, ldq, scale, M, K);
}

void launch_layernorm_q8(const void* x, const void* r, void* sum_out, const void* w, const void* b, void* q,
                         float* scale, int M, int H, float eps, hipStream_t s) {
  launch_norm_q8_t<false>(x, r, sum_out, w, b, q, scale, M, H, eps, s);
}

void launch_rmsnorm_q8(const void* x, const void* r, void* sum_out, const void* w, void* q, float* scale, int M,
                       int H, float eps, hipStream_t s) {
  launch_norm_q8_t<true>(x, r, sum_out, w, nullptr, q, scale, M, H, eps, s);
}
