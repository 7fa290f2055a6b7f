// Row-group geometry of the kernels that walk rows of C entries (dirichlet.hip, mixture.hip): one
// (particle, row) per group of W = min(64, next_pow2(C)) lanes, lanes striding over the entries, row
// reductions by __shfl_xor inside the group -- many small rows share a wave, a C = 1024 row is one
// wave looping 16 times. Every reduction has a fixed order, so results do not depend on the launch.
#pragma once

#include "common.hpp"
#include "device_math.hpp"
#include "internal.hpp"

namespace mi {

constexpr int kRowThreads = 256;

// Sum over the W lanes of a row group (W a power of two <= 64; groups are W-aligned, so the
// exchange partners stay inside the group). Every lane of the wave must be active.
template <typename T>
MI_DEV T group_sum(T v, int W) {
  for (int offset = W >> 1; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, kWave);
  return v;
}

// Maximum over the W lanes of a row group (fmaxf: a NaN lane is ignored).
MI_DEV float group_max(float v, int W) {
  for (int offset = W >> 1; offset > 0; offset >>= 1) v = fmaxf(v, __shfl_xor(v, offset, kWave));
  return v;
}

// The row a lane works on: wave w of the launch holds rows [w * G, w * G + G), G = 64 / W.
struct RowLane {
  int sub;       // lane within the row group: entries sub, sub + W, ...
  int64_t row;   // row index
};

MI_DEV RowLane row_lane(int shift) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kRowThreads / kWave) + (threadIdx.x >> 6);
  return RowLane{lane & ((1 << shift) - 1), wave * (kWave >> shift) + (lane >> shift)};
}

// total[k] = scale * sum_i row_lp[k, i]: one wave per particle, lanes striding over rows, fp64.
static __global__ __launch_bounds__(kRowThreads) void k_rows_finalize(
    const double* __restrict__ row_lp, int64_t K, int64_t N, double scale,
    float* __restrict__ total) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t k = (int64_t)blockIdx.x * (kRowThreads / kWave) + (threadIdx.x >> 6);
  double acc = 0.0;
  if (k < K)
    for (int64_t i = lane; i < N; i += kWave) acc += row_lp[k * N + i];
  acc = wave_sum(acc);
  if (k < K && lane == 0) total[k] = (float)(acc * scale);
}

}  // namespace mi

// Lanes per row: min(64, next_pow2(C)), and its log2.
inline void row_group(int64_t C, int* W, int* shift) {
  int w = 1, s = 0;
  while (w < 64 && w < C) {
    w <<= 1;
    ++s;
  }
  *W = w;
  *shift = s;
}

// Blocks of a row-walking launch over `rows` rows (0: more than a grid holds).
inline int64_t row_blocks(int64_t rows, int W) {
  const int64_t waves = ceil_div(rows, 64 / W);
  const int64_t blocks = ceil_div(waves, mi::kRowThreads / 64);
  return blocks <= kMaxGrid ? blocks : 0;
}

// K, N, C >= 1 with K * N * C elements (and their byte offsets) inside int64.
inline bool row_shape_ok(int64_t K, int64_t N, int64_t C) {
  return K >= 1 && N >= 1 && C >= 1 && K <= (INT64_MAX / 8) / N && K * N <= (INT64_MAX / 8) / C;
}
