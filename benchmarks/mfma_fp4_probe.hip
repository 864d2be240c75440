// Lane maps of the mixed fp4 x fp8 block-scaled MFMA (MI355X): v_mfma_scale_f32_16x16x128_f8f6f4
// with cbsz = 4 (first operand e2m1, four VGPRs) and blgp = 0 (second operand e4m3, eight VGPRs).
// One wave answers three questions csrc/kernels/gemm_w4a8.hip depends on:
//   1. which k does each register position hold? Hypothesis: an fp4 lane (l16, g = lane >> 4) holds
//      row l16, k = 32g + e, element e the low (e even) / high (e odd) nibble of byte e/2 of its 16
//      bytes; an e4m3 lane (l16, g) holds k = 16g + i in byte i < 16 of its 32 and k = 64 + 16g +
//      (i - 16) in byte i >= 16: two 16-byte halves, NOT 32 consecutive k.
//   2. which lane's scale applies: that of lane (l16, g) to row l16, k = 32g .. 32g+31?
//   3. which byte of the scale VGPR does op_sel = j select? Hypothesis: byte j.
// W holds distinct non-zero e2m1 codes and a distinct e8m0 code per (row, block, scale byte); the
// activations are one-hot (1.0 at k = (t + c) % 128 for column c of pass t), so every output is one
// decoded weight times one scale, and a mismatch names the element and the scale that were used.
// Two code patterns are run: together (k % 14, (k % 32) / 14) identify k inside a block.
// Prints, per pattern and op_sel, how many of 128 x 256 outputs differ from the hypothesis.
// Measured: 0 differ. (With the e4m3 lane holding k = 32g + i instead, 24576 of 32768 differ: only
// bytes 0..15 of lane group 0 and 16..31 of lane group 3 keep their k.)
//
//   hipcc -O2 --offload-arch=gfx950 benchmarks/mfma_fp4_probe.hip -o build/mfma_fp4_probe && build/mfma_fp4_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPasses = 128;

// W [16][64] bytes (two e2m1 per byte), S [16][4 blocks][4 bytes] e8m0, out [kPasses][16 rows][16 cols]
template <int SEL>
__global__ void probe(const uint8_t* W, const uint8_t* S, float* out) {
  const int lane = threadIdx.x, l16 = lane & 15, g = lane >> 4;
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const int*>(W + l16 * 64 + g * 16 + i * 4);
  const int sc = *reinterpret_cast<const int*>(S + (l16 * 4 + g) * 4);
  for (int t = 0; t < kPasses; ++t) {
    // column l16 is one-hot at k = (t + l16) % 128: lane group (k / 16) % 4, byte 16 * (k / 64) + k % 16
    const int k = (t + l16) & 127, i = 16 * (k >> 6) + (k & 15);
    i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
    if (((k >> 4) & 3) == g) b[i >> 2] = 0x38 << (8 * (i & 3));  // e4m3 1.0
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 4, 0, SEL, sc, 0, 0x7f7f7f7f);
    // D[row 4g + i][col l16]: row <-> W row, col <-> activation row
    for (int i = 0; i < 4; ++i) out[(t * 16 + 4 * g + i) * 16 + l16] = d[i];
  }
}

static float dec4(int c) {
  static const float v[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  return (c & 8) ? -v[c & 7] : v[c & 7];
}

int main() {
  static const int nz[14] = {1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15};
  uint8_t *dW, *dS;
  float* dO;
  if (hipMalloc(&dW, 16 * 64) != hipSuccess || hipMalloc(&dS, 256) != hipSuccess ||
      hipMalloc(&dO, kPasses * 256 * 4) != hipSuccess)
    return 2;
  // scale byte j of (row r, block b): distinct over (b, j) and shifted per row, 2^-16 .. 2^47
  std::vector<uint8_t> S(256);
  for (int r = 0; r < 16; ++r)
    for (int b = 0; b < 4; ++b)
      for (int j = 0; j < 4; ++j) S[(r * 4 + b) * 4 + j] = (uint8_t)(111 + (r + 4 * b) % 16 + 16 * j);
  (void)hipMemcpy(dS, S.data(), S.size(), hipMemcpyHostToDevice);
  int total_bad = 0;
  for (int pat = 0; pat < 2; ++pat) {
    std::vector<int> code(16 * 128);
    std::vector<uint8_t> W(16 * 64, 0);
    for (int r = 0; r < 16; ++r)
      for (int k = 0; k < 128; ++k) {
        const int c = nz[pat == 0 ? (k + r) % 14 : ((k % 32) / 14 + 5 * (k / 32) + r) % 14];
        code[r * 128 + k] = c;
        W[r * 64 + k / 2] |= (uint8_t)(c << (4 * (k & 1)));  // even k: low nibble
      }
    (void)hipMemcpy(dW, W.data(), W.size(), hipMemcpyHostToDevice);
    for (int sel = 0; sel < 4; ++sel) {
      (void)hipMemset(dO, 0, kPasses * 256 * 4);
      if (sel == 0) hipLaunchKernelGGL(probe<0>, dim3(1), dim3(64), 0, 0, dW, dS, dO);
      if (sel == 1) hipLaunchKernelGGL(probe<1>, dim3(1), dim3(64), 0, 0, dW, dS, dO);
      if (sel == 2) hipLaunchKernelGGL(probe<2>, dim3(1), dim3(64), 0, 0, dW, dS, dO);
      if (sel == 3) hipLaunchKernelGGL(probe<3>, dim3(1), dim3(64), 0, 0, dW, dS, dO);
      if (hipDeviceSynchronize() != hipSuccess) return 3;
      std::vector<float> O(kPasses * 256);
      (void)hipMemcpy(O.data(), dO, O.size() * 4, hipMemcpyDeviceToHost);
      int bad = 0;
      for (int t = 0; t < kPasses; ++t)
        for (int r = 0; r < 16; ++r)
          for (int c = 0; c < 16; ++c) {
            const int k = (t + c) & 127;
            const float want = std::ldexp(dec4(code[r * 128 + k]), S[(r * 4 + k / 32) * 4 + sel] - 127);
            const float got = O[(t * 16 + r) * 16 + c];
            if (want == got) continue;
            if (bad < 4) {
              // which (element, scale byte) of the row explains the value?
              int fk = -1, fj = -1, fb = -1;
              for (int k2 = 0; k2 < 128 && fk < 0; ++k2)
                for (int b2 = 0; b2 < 4 && fk < 0; ++b2)
                  for (int j2 = 0; j2 < 4 && fk < 0; ++j2)
                    if (std::ldexp(dec4(code[r * 128 + k2]), S[(r * 4 + b2) * 4 + j2] - 127) == got)
                      fk = k2, fb = b2, fj = j2;
              printf("  pattern %d op_sel %d row %d k %d: got %g want %g (first match: element %d, scale of block %d byte %d)\n",
                     pat, sel, r, k, got, want, fk, fb, fj);
            }
            ++bad;
          }
      printf("pattern %d op_sel %d: %d of %d differ from the hypothesis\n", pat, sel, bad, kPasses * 256);
      total_bad += bad;
    }
  }
  printf("%s\n", total_bad ? "HYPOTHESIS REFUTED" : "hypothesis holds: fp4 k = 32g + e, low nibble first; e4m3 halves at k = 16g and 64 + 16g; op_sel j = scale byte j");
  return 0;
}
