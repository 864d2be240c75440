// Lane <-> element layout of the transposed LDS reads of CDNA4 (MI355X): ds_read_b64_tr_b16, which
// csrc/kernels/attention_impl.h, attn_decode.hip and attn_decode_fp8.hip build their V^T fragments
// on, and ds_read_b64_tr_b8, the 8-bit form an e4m3 V^T fragment could use instead of the fp8
// kernel's byte-pair read plus v_perm_b32. One wave; lane l passes the address of ITS OWN 8 bytes
// (row l of a [64][8]-byte matrix), so an element of the result is named by the lane whose address
// supplied it and its index inside that lane's 8 bytes. Two passes tell the two apart: the bytes
// hold the lane number, then the index.
//
// b16: the probe CHECKS the layout the kernels assume — element j (of 4 x 16 bit) of lane 16k + li
// is element li & 3 of the 8 bytes addressed by lane 16k + 4j + (li >> 2): within 16 lanes, lane
// (q, p) addresses row q, columns 4p .. 4p+3 of a 4 x 16 block and lane li receives column li.
// b8: the probe PRINTS the layout and checks that it is a permutation inside each group of 16
// lanes. Measured on an MI355X: see profiles/decode_fp8/ds_read_tr8_probe.txt.
//
//   hipcc -O2 --offload-arch=gfx950 benchmarks/ds_read_tr8_probe.hip -o build/ds_read_tr8_probe && build/ds_read_tr8_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;

// out [2 passes][2 forms][64 lanes][8 bytes]
__global__ void probe(uint8_t* out) {
  __shared__ __attribute__((aligned(16))) uint8_t m[64 * 8];
  const int lane = threadIdx.x;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < 8; ++i) m[lane * 8 + i] = pass == 0 ? lane : i;
    __syncthreads();
    const i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(m + lane * 8));
    const i32x2 b = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(m + lane * 8));
    __syncthreads();
    *reinterpret_cast<i16x4*>(out + ((pass * 2 + 0) * 64 + lane) * 8) = a;
    *reinterpret_cast<i32x2*>(out + ((pass * 2 + 1) * 64 + lane) * 8) = b;
  }
}

int main() {
  uint8_t* d;
  if (hipMalloc(&d, 2 * 2 * 64 * 8) != hipSuccess) return 2;
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  std::vector<uint8_t> o(2 * 2 * 64 * 8);
  hipMemcpy(o.data(), d, o.size(), hipMemcpyDeviceToHost);
  auto at = [&](int pass, int form, int lane, int i) { return (int)o[((pass * 2 + form) * 64 + lane) * 8 + i]; };
  int bad16 = 0;
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 4; ++j)
      for (int h = 0; h < 2; ++h) {  // the two bytes of 16-bit element j
        const int li = l & 15, src = (l & 48) + 4 * j + (li >> 2), idx = 2 * (li & 3) + h;
        bad16 += at(0, 0, l, 2 * j + h) != src || at(1, 0, l, 2 * j + h) != idx;
      }
  printf("ds_read_b64_tr_b16: %d of 512 bytes differ from the layout the attention kernels assume\n", bad16);
  printf("ds_read_b64_tr_b8: byte j of lane l <- (lane whose address supplied it).(byte of its 8)\n");
  int bad8 = 0;
  for (int l = 0; l < 64; ++l) {
    printf("lane %2d:", l);
    for (int j = 0; j < 8; ++j) {
      printf(" %2d.%d", at(0, 1, l, j), at(1, 1, l, j));
      bad8 += (at(0, 1, l, j) & 48) != (l & 48);
    }
    printf("\n");
  }
  std::vector<int> seen(512, 0);
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 8; ++j) seen[at(0, 1, l, j) * 8 + at(1, 1, l, j)]++;
  for (int s : seen) bad8 += s != 1;
  printf("ds_read_b64_tr_b8: %s inside each group of 16 lanes\n", bad8 ? "NOT a permutation" : "a permutation");
  return bad16 || bad8 ? 1 : 0;
}
