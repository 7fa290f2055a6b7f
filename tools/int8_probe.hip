// The two bare matrix loops of k_site_bcast_smem at the kernel's shape, timed against each other:
// one wave's 12 independent accumulators (4 column tiles x 3 pieces) per ds_read_b128, a 4096-element
// 0/1 chunk as 8 bf16 fragments (v_mfma_f32_16x16x32_bf16) or 4 int8 fragments
// (v_mfma_i32_16x16x64_i8), accumulators zeroed per chunk, the s_nop pair and a read-out behind
// every chunk. 768 workgroups of four waves: three waves per SIMD on 256 CUs. Prints the time and
// the shader clocks of one chunk per wave, and checks the sums. Not used by the library.
// clocks_per_mfma_per_simd divides by the waves per SIMD of a 256-CU device (workgroups / 256).
//   hipcc -O3 --offload-arch=gfx950 tools/int8_probe.hip -o tools/int8_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kChunk = 4096, kThreads = 256;

#define CHECK(call) \
  do { \
    const hipError_t e_ = (call); \
    if (e_ != hipSuccess) { \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); \
      exit(1); \
    } \
  } while (0)

// out[workgroup * 256 + thread]: the sum over the wave's chunks of the 12 accumulators' elements.
template <bool INT8>
__global__ __launch_bounds__(kThreads) void k_loop(int chunks, int nf, int b_word, double* __restrict__ out,
                                                   unsigned long long* __restrict__ clocks) {
  constexpr int kBytes = INT8 ? kChunk : 2 * kChunk;
  // (nf: the chunk's fragments, 64 lanes x 16 bytes each; an argument, so the loop stays a loop)
  __shared__ __attribute__((aligned(16))) unsigned char xa[kBytes];
  // every third element is a one
  for (int e = threadIdx.x; e < kChunk; e += kThreads) {
    const bool one = e % 3 == 0;
    if (INT8) xa[e] = one ? 1 : 0;
    else reinterpret_cast<unsigned short*>(xa)[e] = one ? 0x3f80 : 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const i32x4* frag = reinterpret_cast<const i32x4*>(xa) + lane;
  i32x4 b[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) b[i] = i32x4{b_word, b_word, b_word, b_word};
  double total = 0.0;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int c = 0; c < chunks; ++c) {
    typedef typename std::conditional<INT8, i32x4, f32x4>::type acc_t;
    acc_t d[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) d[i] = acc_t{0, 0, 0, 0};
    int f = 0;
    i32x4 next = frag[0];
    do {
      const i32x4 a = next;
      next = frag[min(f + 1, nf - 1) * 64];
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        if (INT8)
          __asm__ volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(d[i]) : "v"(a), "v"(b[i]));
        else
          __asm__ volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(d[i]) : "v"(a), "v"(b[i]));
      }
    } while (++f < nf);
    __asm__ volatile("s_nop 15\n\ts_nop 15"
                     : "+a"(d[0]), "+a"(d[1]), "+a"(d[2]), "+a"(d[3]), "+a"(d[4]), "+a"(d[5]),
                       "+a"(d[6]), "+a"(d[7]), "+a"(d[8]), "+a"(d[9]), "+a"(d[10]), "+a"(d[11]));
#pragma unroll
    for (int i = 0; i < 12; ++i) total += (double)((d[i].x + d[i].y) + (d[i].z + d[i].w));
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  out[(size_t)blockIdx.x * kThreads + threadIdx.x] = total;
  if (lane == 0) clocks[blockIdx.x * (kThreads / 64) + threadIdx.x / 64] = t1 - t0;
}

template <bool INT8>
void run(const char* name, int grid, int chunks, double* out, unsigned long long* clocks) {
  // B: 1.0 in bf16, 1 in every byte for int8, so a lane's four accumulator elements of a tile add
  // up to the ones among the 4 rows x (32 or 64) k it holds, and all 64 lanes to the chunk's 1366.
  const int frags = INT8 ? 4 : 8;
  const int b_word = INT8 ? 0x01010101 : 0x3f803f80;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int w = 0; w < 3; ++w) hipLaunchKernelGGL(k_loop<INT8>, dim3(grid), dim3(kThreads), 0, 0, chunks, frags, b_word, out, clocks);
  CHECK(hipGetLastError());
  float best = 1e30f;
  for (int r = 0; r < 5; ++r) {
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_loop<INT8>, dim3(grid), dim3(kThreads), 0, 0, chunks, frags, b_word, out, clocks);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    best = ms < best ? ms : best;
  }
  std::vector<double> h((size_t)grid * kThreads);
  std::vector<unsigned long long> hc((size_t)grid * (kThreads / 64));
  CHECK(hipMemcpy(h.data(), out, h.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hc.data(), clocks, hc.size() * 8, hipMemcpyDeviceToHost));
  bool ok = true;
  for (size_t w = 0; w < h.size() / 64; ++w) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += h[w * 64 + l];
    // per chunk: 12 tiles x 16 columns x 1366 ones, each tile column summed over all rows
    ok = ok && s == 12.0 * 16.0 * 1366.0 * chunks;
  }
  double clk = 0.0;
  for (unsigned long long c : hc) clk += (double)c;
  clk /= (double)hc.size();
  printf("{\"loop\": \"%s\", \"workgroups\": %d, \"chunks_per_wave\": %d, \"us_per_chunk\": %.4f, "
         "\"clocks_per_chunk\": %.1f, \"clocks_per_mfma_per_simd\": %.2f, \"sums_ok\": %s}\n",
         name, grid, chunks, 1e3 * best / chunks, clk / chunks,
         clk / chunks / (12.0 * frags) / (grid / 256.0 > 1.0 ? grid / 256.0 : 1.0), ok ? "true" : "false");
}

int main() {
  const int chunks = 2000;
  double* out;
  unsigned long long* clocks;
  CHECK(hipMalloc(&out, (size_t)768 * kThreads * 8));
  CHECK(hipMalloc(&clocks, (size_t)768 * 4 * 8));
  for (int rep = 0; rep < 2; ++rep)
    for (int grid : {256, 512, 768}) {   // one, two, three waves per SIMD
      run<false>("bf16 16x16x32, 8 fragments", grid, chunks, out, clocks);
      run<true>("int8 16x16x64, 4 fragments", grid, chunks, out, clocks);
    }
  return 0;
}
