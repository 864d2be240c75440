// In-kernel phase timing of one LDS-DMA GEMM config (diagnostic executable): compiles
// csrc/kernels/gemm_glds_impl.h (configs 34, 13, 24, 27, 17, 45, 25, 22, and the wave-private
// rings 120..123: W x S = 8 x 2, 4 x 3, 6 x 2, 12 x 1, and on 64-row tiles 130..133: 64 x 96 at
// 4 x 2 and 3 x 2, 64 x 80 at 4 x 2 and 3 x 2, epilogues ln / lngelu only) into this translation unit
// with DLS_STAMP recording s_memrealtime (100 MHz) per workgroup at: tile start, after the main
// loop (1), after the K groups' fragments are summed or, on the one-pass configs (Cfg::ONE_PASS),
// handed over through LDS (7), after the output image is in LDS (2; the one-pass finish has no
// image and never stamps it), after the stores (3). On the wave-private rings stamp 1 is WAVE 0's
// own K loop (the waves do not meet inside it) and stamp 7 follows the kernel's one barrier, so
// "main loop" + "K groups > LDS" is the figure to set against a K-grouped config's.
//
// The epilogue mode attaches the operands a model step attaches (none: a bare GEMM):
//   res     bias + residual + stats_out            (GPT-2 out-proj, fc2)
//   lngelu  bias + ln_colsum + ext_stats, GeLU     (fc1: folded LayerNorm, external statistics)
//   ln      bias + ln_colsum + ext_stats           (QKV, LM head)
// The operands are written by earlier launches, as in a step. The stamps in the middle of the
// epilogue wait for the stamping wave's LDS traffic only (a vmcnt(0) there would drain operand
// requests that are meant to be in flight across the phase boundary).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -Icsrc/kernels \
//         benchmarks/gemm_stamps.hip -o gpubin/gemm_stamps
//   gpubin/gemm_stamps <cfg> <M> <N> <K> [none|res|lngelu|ln] [stream_pol]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

constexpr int kMaxBlocks = 4096, kSlots = 8;
__device__ unsigned long long g_stamps[kMaxBlocks * kSlots];
#define DLS_STAMP(k)                                                                     \
  if (threadIdx.x == 0 && blockIdx.x < kMaxBlocks) {                                     \
    if ((k) == 0 || (k) == 3) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                              \
    g_stamps[blockIdx.x * kSlots + (k)] = __builtin_amdgcn_s_memrealtime();              \
  }
#include "gemm_glds_impl.h"
DLS_GLDS_DEFINE(34)
DLS_GLDS_DEFINE(13)
DLS_GLDS_DEFINE(24)
DLS_GLDS_DEFINE(27)
DLS_GLDS_DEFINE(17)
DLS_GLDS_DEFINE(45)
DLS_GLDS_DEFINE(25)
DLS_GLDS_DEFINE(22)
// splitk = 1 only: the split-K reduce launcher of the library is stubbed out below
static bool launch_gemm_glds_local(const GemmArgs& a, int cfg, const float* colsum, int ln_mode) {
  if (cfg >= kGemmPrivateWide) {
    const int waves = cfg < kGemmPrivateWide + kGemmPrivateWideCount ? kGemmPrivateWideCfgs[cfg - kGemmPrivateWide].waves : 0;
    if (!colsum || !private_wide_takes(waves, a, 1, ln_mode, false)) {
      fprintf(stderr, "config %d does not take this shape / epilogue\n", cfg);
      exit(2);
    }
    if (cfg == 130) launch_private_wide<64, 96, 4, 2>(a, colsum, ln_mode, 1e-5f, 0);
    else if (cfg == 131) launch_private_wide<64, 96, 3, 2>(a, colsum, ln_mode, 1e-5f, 0);
    else if (cfg == 132) launch_private_wide<64, 80, 4, 2>(a, colsum, ln_mode, 1e-5f, 0);
    else launch_private_wide<64, 80, 3, 2>(a, colsum, ln_mode, 1e-5f, 0);
    return false;
  }
  if (cfg >= 120) {
    const int waves = cfg == 120 ? 8 : cfg == 121 ? 4 : cfg == 122 ? 6 : cfg == 123 ? 12 : 0;
    const bool ok = private_takes(waves, a, 1, ln_mode != 0, false);
    if (!ok) {
      fprintf(stderr, "config %d does not take this shape / epilogue\n", cfg);
      exit(2);
    }
    if (cfg == 120) launch_private<8, 2>(a, 0);
    else if (cfg == 121) launch_private<4, 3>(a, 0);
    else if (cfg == 122) launch_private<6, 2>(a, 0);
    else launch_private<12, 1>(a, 0);
    return false;
  }
  switch (cfg) {
    case 13: return glds_launch_cfg13(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 24: return glds_launch_cfg24(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 27: return glds_launch_cfg27(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 17: return glds_launch_cfg17(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 45: return glds_launch_cfg45(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 25: return glds_launch_cfg25(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    case 22: return glds_launch_cfg22(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
    default: return glds_launch_cfg34(a, 1, nullptr, 0, colsum, ln_mode, 1e-5f, nullptr, false);
  }
}
bool glds_reduce(const GemmArgs&, int, float*, hipStream_t, const float*, int, float, const int*, const Epi&) { return false; }

int main(int argc, char** argv) {
  const int cfg = argc > 1 ? atoi(argv[1]) : 34;
  const int M = argc > 2 ? atoi(argv[2]) : 512, N = argc > 3 ? atoi(argv[3]) : 32768, K = argc > 4 ? atoi(argv[4]) : 768;
  const char* mode = argc > 5 ? argv[5] : "none";
  const bool res = !strcmp(mode, "res"), ln = !strcmp(mode, "ln") || !strcmp(mode, "lngelu");
  if (!res && !ln && strcmp(mode, "none")) {
    fprintf(stderr, "epilogue mode: none, res, lngelu or ln\n");
    return 2;
  }
  std::vector<unsigned short> h(std::max({(size_t)M * K, (size_t)N * K, (size_t)M * N}));
  for (size_t i = 0; i < h.size(); ++i) h[i] = 0x3c00 + (unsigned short)(rand() & 0x3ff);  // bf16 in [1, 2)
  void *A, *W, *C, *B, *R;
  float *colsum, *ext, *stats;
  hipMalloc(&A, (size_t)M * K * 2);
  hipMalloc(&W, (size_t)N * K * 2);
  hipMalloc(&C, (size_t)M * N * 2);
  hipMalloc(&B, (size_t)N * 2);
  hipMalloc(&R, (size_t)M * N * 2);
  hipMalloc(&colsum, (size_t)N * 4);
  hipMalloc(&ext, (size_t)M * 2 * 4);
  hipMalloc(&stats, (size_t)M * 2 * 4);
  hipMemcpy(A, h.data(), (size_t)M * K * 2, hipMemcpyHostToDevice);
  hipMemcpy(W, h.data(), (size_t)N * K * 2, hipMemcpyHostToDevice);
  hipMemcpy(B, h.data(), (size_t)N * 2, hipMemcpyHostToDevice);
  hipMemcpy(R, h.data(), (size_t)M * N * 2, hipMemcpyHostToDevice);
  // statistics of rows whose values have mean 1.5 and mean square 2.5 (a positive variance)
  std::vector<float> f((size_t)std::max(2 * M, N));
  for (int i = 0; i < M; ++i) {
    f[2 * i] = 1.5f * K;
    f[2 * i + 1] = 2.5f * K;
  }
  hipMemcpy(ext, f.data(), (size_t)M * 2 * 4, hipMemcpyHostToDevice);
  for (int i = 0; i < N; ++i) f[i] = 1.5f * K;
  hipMemcpy(colsum, f.data(), (size_t)N * 4, hipMemcpyHostToDevice);
  hipMemset(stats, 0, (size_t)M * 2 * 4);
  GemmArgs g{};
  g.A = A; g.lda = K; g.W = W; g.ldw = K; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.alpha = 1.f;
  g.config = cfg;
  g.stream_pol = argc > 6 ? atoi(argv[6]) : 0;
  if (res) {
    g.bias = B; g.R = R; g.ldr = N; g.stats_out = stats;
  } else if (ln) {
    g.bias = B; g.ext_stats = ext;
    g.act = !strcmp(mode, "lngelu") ? ACT_GELU_TANH : ACT_NONE;
  }
  const float* cs = ln ? colsum : nullptr;
  const int ln_mode = ln ? 1 : 0;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipMemset(C, 0, (size_t)M * N * 2);
  for (int i = 0; i < 5; ++i) launch_gemm_glds_local(g, cfg, cs, ln_mode);
  hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), std::vector<unsigned long long>(kMaxBlocks * kSlots, 0).data(),
                    kMaxBlocks * kSlots * 8);
  hipEventRecord(e0);
  launch_gemm_glds_local(g, cfg, cs, ln_mode);
  hipEventRecord(e1);
  if (hipEventSynchronize(e1) != hipSuccess) {
    fprintf(stderr, "launch failed: %s\n", hipGetErrorString(hipGetLastError()));
    return 1;
  }
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> st(kMaxBlocks * kSlots);
  hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_stamps), st.size() * 8);
  unsigned long long t0 = ~0ull, tend = 0;
  for (int b = 0; b < kMaxBlocks; ++b) {
    const unsigned long long* s = &st[b * kSlots];
    if (!s[0]) continue;
    t0 = std::min(t0, s[0]);
    tend = std::max(tend, s[3]);
  }
  // phases: 0 -> 1 main loop, 1 -> 7 K groups through LDS (staged: group 0 holds their sum;
  // one-pass: every group's fragments are in LDS), 7 -> 2 image (staged only), 2 -> 3 finish and
  // store (staged: the store pass; one-pass: sum, epilogue and store — from stamp 7)
  std::vector<double> d_main, d_sum, d_img, d_store, d_epi, start, end;
  for (int b = 0; b < kMaxBlocks; ++b) {
    const unsigned long long* s = &st[b * kSlots];
    if (!s[0]) continue;
    d_main.push_back((s[1] - s[0]) * 0.01);
    d_sum.push_back((s[7] - s[1]) * 0.01);
    const unsigned long long s2 = s[2] ? s[2] : s[7];  // (one-pass: no image phase)
    d_img.push_back((s2 - s[7]) * 0.01);
    d_store.push_back((s[3] - s2) * 0.01);
    d_epi.push_back((s[3] - s[1]) * 0.01);
    start.push_back((s[0] - t0) * 0.01);
    end.push_back((s[3] - t0) * 0.01);
  }
  auto q = [](std::vector<double> v, double p) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[(size_t)(p * (v.size() - 1))];
  };
  auto mean = [](const std::vector<double>& v) {
    double s = 0;
    for (double x : v) s += x;
    return v.empty() ? 0.0 : s / v.size();
  };
  printf("cfg %d  M %d N %d K %d  epilogue %s: event %.2f us; blocks %zu; first-start -> last-end %.2f us\n", cfg, M,
         N, K, mode, ms * 1e3, d_main.size(), (tend - t0) * 0.01);
  printf("  start offset   min %.2f med %.2f max %.2f us\n", q(start, 0), q(start, .5), q(start, 1));
  printf("  main loop      min %.2f med %.2f max %.2f mean %.2f us\n", q(d_main, 0), q(d_main, .5), q(d_main, 1), mean(d_main));
  printf("  K groups > LDS min %.2f med %.2f max %.2f mean %.2f us\n", q(d_sum, 0), q(d_sum, .5), q(d_sum, 1), mean(d_sum));
  printf("  image to LDS   min %.2f med %.2f max %.2f mean %.2f us\n", q(d_img, 0), q(d_img, .5), q(d_img, 1), mean(d_img));
  printf("  finish + store min %.2f med %.2f max %.2f mean %.2f us\n", q(d_store, 0), q(d_store, .5), q(d_store, 1), mean(d_store));
  printf("  after the loop min %.2f med %.2f max %.2f mean %.2f us\n", q(d_epi, 0), q(d_epi, .5), q(d_epi, 1), mean(d_epi));
  printf("  end offset     min %.2f med %.2f max %.2f us\n", q(end, 0), q(end, .5), q(end, 1));
  return 0;
}
