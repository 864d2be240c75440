// Neutral block scale of the f8f6f4 MFMA (MI355X): does v_mfma[_scale]_f32_16x16x128_f8f6f4 with
// e4m3 operands multiply by exactly 1 with literal-zero scale arguments (the compiler then selects
// the unscaled encoding) and with 0x7f7f7f7f (scaled encoding, e8m0 1.0 in every byte)? One wave:
// A holds every finite e4m3 code, B is one-hot (1.0 at k = 8c + t for column c, pass t), so
// D[r][c] must be the decoded A[r][8c + t] bit for bit. Both operands of a lane group come from the
// same byte range of their rows, as in csrc/kernels/gemm_w8a8.hip, so no k map is assumed.
// Measured: 0 of 2048 values differ in either form.
//
//   hipcc -O2 --offload-arch=gfx950 benchmarks/mfma_scale_probe.hip -o build/mfma_scale_probe && build/mfma_scale_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// A [16][128] bytes, B [8][16][128] bytes, out [2][8][16 rows][16 cols]
__global__ void probe(const uint8_t* A, const uint8_t* B, float* out) {
  const int lane = threadIdx.x, l16 = lane & 15, g = lane >> 4;
  i32x8 a;
  for (int i = 0; i < 8; ++i) a[i] = *reinterpret_cast<const int*>(A + l16 * 128 + g * 32 + i * 4);
  for (int t = 0; t < 8; ++t) {
    i32x8 b;
    for (int i = 0; i < 8; ++i) b[i] = *reinterpret_cast<const int*>(B + (t * 16 + l16) * 128 + g * 32 + i * 4);
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 d0 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 0, 0, 0, 0, 0, 0);
    f32x4 d1 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    // D[row 4g + i][col l16]: row <-> A row, col <-> B row
    for (int i = 0; i < 4; ++i) {
      out[((0 * 8 + t) * 16 + 4 * g + i) * 16 + l16] = d0[i];
      out[((1 * 8 + t) * 16 + 4 * g + i) * 16 + l16] = d1[i];
    }
  }
}

static float dec(uint8_t c) {
  const int s = c >> 7, e = (c >> 3) & 15, m = c & 7;
  const float v = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.0f + m / 8.0f, e - 7);
  return s ? -v : v;
}

int main() {
  std::vector<uint8_t> codes;
  for (int c = 0; c < 256; ++c)
    if ((c & 0x7f) != 0x7f) codes.push_back((uint8_t)c);
  std::vector<uint8_t> A(16 * 128), B(8 * 16 * 128, 0);
  for (int r = 0; r < 16; ++r)
    for (int k = 0; k < 128; ++k) A[r * 128 + k] = codes[(r * 17 + k) % 254];
  for (int t = 0; t < 8; ++t)
    for (int c = 0; c < 16; ++c) B[(t * 16 + c) * 128 + c * 8 + t] = 0x38;  // 1.0 at k = 8c + t
  uint8_t *dA, *dB;
  float* dO;
  if (hipMalloc(&dA, A.size()) != hipSuccess || hipMalloc(&dB, B.size()) != hipSuccess ||
      hipMalloc(&dO, 2 * 8 * 256 * 4) != hipSuccess)
    return 2;
  hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
  hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dO);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  std::vector<float> O(2 * 8 * 256);
  hipMemcpy(O.data(), dO, O.size() * 4, hipMemcpyDeviceToHost);
  for (int f = 0; f < 2; ++f) {
    int bad = 0;
    float first_got = 0, first_want = 0;
    for (int t = 0; t < 8; ++t)
      for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) {
          const float want = dec(A[r * 128 + c * 8 + t]), got = O[((f * 8 + t) * 16 + r) * 16 + c];
          if (!(want == got)) {
            if (!bad) first_got = got, first_want = want;
            ++bad;
          }
        }
    printf("%s: %d of 2048 differ (first: got %g want %g)\n", f ? "scale 0x7f7f7f7f (scaled encoding)" : "scale literal 0 (unscaled encoding)",
           bad, first_got, first_want);
  }
  return 0;
}
