// Entropy of a LowRankMultivariateNormal guide factor and its gradient.
//
// Replaces LowRankMultivariateNormal.entropy() (torch 2.10 lowrank_multivariate_normal.py:225-237)
// and the gradients autograd computes through the constructor's capacitance product and Cholesky,
// for W = cov_factor[D, R], d = cov_diag[D] and L = _capacitance_tril[R, R], the lower factor of
// C = I + W^T diag(1 / d) W. With M = W C^-1:
//   H         = 0.5 D (1 + log 2 pi) + sum_j log L[j, j] + 0.5 sum_i log d[i]
//   dH/dW[i, r] = M[i, r] / d[i]
//   dH/dd[i]    = 0.5 (1 / d[i] - (sum_r M[i, r] W[i, r]) / d[i]^2)
// Three launches:
//   1. one workgroup, fp64 in LDS: L^-1 by right-looking forward substitution, C^-1 = L^-T L^-1
//      (f32, full and exactly symmetric) and sum_j log L[j, j] into the workspace;
//   2. the row pass: M = W C^-1 with the row-wise epilogue above and one fp64 partial of
//      sum_i log d[i] per block. R >= 32: v_mfma_f32_32x32x2_f32 over the 32 x 32 tiles of
//      mfma_tile.hpp, a wave per tile of 32 rows, C^-1 staged once per block. R < 32: on the VALU, a
//      thread per row with the rank padded to 4, 8, 16 or 32 (lowrank_guide.hip says why);
//   3. the partials summed in block order in fp64, and the value.
// Without gradient outputs launch 1 only sums the logs and launch 2 only log d. Every sum has a
// fixed order (no atomics): two calls on the same inputs are bit-identical.
#include "internal.hpp"
#include "lowrank_capacitance.hpp"
#include "mfma_tile.hpp"

#include <algorithm>

namespace mi {

constexpr int kLeRowThreads = 256;         // the VALU row pass: a row per thread
constexpr int kLeSumThreads = 256;         // the finish

// ---- 1. the R x R stage (lowrank_capacitance.hpp) -----------------------------------------------
__global__ __launch_bounds__(1024) void k_lowrank_entropy_capacitance(
    const float* __restrict__ L, int R, int inverse, float* __restrict__ cinv,
    double* __restrict__ logdet) {
  extern __shared__ double X[];   // [R][ld], then the R logs
  const int ld = R | 1;
  double* lg = X + R * ld;
  const int t = threadIdx.x, nt = blockDim.x;
  for (int j = t; j < R; j += nt) lg[j] = log((double)L[j * R + j]);
  if (inverse) capacitance_stage(L, R, X);
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < R; ++j) s += lg[j];
    *logdet = s;
  }
  if (!inverse) return;   // (block-uniform)
  capacitance_invert(X, R, cinv);
}

// The block's fp64 sum, threads in a fixed tree: partial[blockIdx.x].
template <int THREADS>
MI_DEV void block_sum_to(double v, double* red, double* __restrict__ partial) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & (kWave - 1)) == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int q = 0; q < THREADS / kWave; ++q) s += red[q];
    partial[blockIdx.x] = s;
  }
}

// ---- 2. the row pass, R < 32: a thread per row, tiles of 256 rows ------------------------------
template <int RQ>
__global__ __launch_bounds__(kLeRowThreads) void k_lowrank_entropy_rows_valu(
    const float* __restrict__ W, const float* __restrict__ d, const float* __restrict__ cinv,
    int64_t D, int64_t R, int64_t tiles, float* __restrict__ dW, float* __restrict__ dd,
    double* __restrict__ partial) {
  constexpr int RP = 4 * RQ;
  __shared__ float cs[RP][RP];
  __shared__ double red[kLeRowThreads / kWave];
  const bool grads = dW != nullptr;
  if (grads) {
    for (int e = threadIdx.x; e < RP * RP; e += kLeRowThreads) {
      const int s = e / RP, r = e - s * RP;
      cs[s][r] = (s < R && r < R) ? cinv[s * R + r] : 0.0f;
    }
  }
  __syncthreads();
  const bool quads = (R & 3) == 0;   // rows of W start on 16 bytes
  double logs = 0.0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kLeRowThreads + threadIdx.x;
    if (i >= D) continue;
    const float di = d[i];
    logs += log((double)di);
    if (!grads) continue;
    float wr[RP], m[RP];
    if (quads) {
#pragma unroll
      for (int q = 0; q < RQ; ++q) {
        const float4 v = 4 * q < R ? *reinterpret_cast<const float4*>(W + i * R + 4 * q)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
        wr[4 * q] = v.x, wr[4 * q + 1] = v.y, wr[4 * q + 2] = v.z, wr[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int r = 0; r < RP; ++r) wr[r] = r < R ? W[i * R + r] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < RP; ++r) m[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < RP; ++s)
#pragma unroll
      for (int r = 0; r < RP; ++r) m[r] = fmaf(wr[s], cs[s][r], m[r]);
    const float inv = 1.0f / di;
    float q = 0.0f;
#pragma unroll
    for (int r = 0; r < RP; ++r) {
      q = fmaf(m[r], wr[r], q);
      m[r] *= inv;
    }
    dd[i] = 0.5f * (inv - q * inv * inv);
    if (quads) {
#pragma unroll
      for (int c = 0; c < RQ; ++c)
        if (4 * c < R)
          *reinterpret_cast<float4*>(dW + i * R + 4 * c) =
              make_float4(m[4 * c], m[4 * c + 1], m[4 * c + 2], m[4 * c + 3]);
    } else {
#pragma unroll
      for (int r = 0; r < RP; ++r)
        if (r < R) dW[i * R + r] = m[r];
    }
  }
  block_sum_to<kLeRowThreads>(logs, red, partial);
}

// ---- 2. the row pass, R >= 32: a wave per tile of 32 rows, groups of four tiles ----------------
// LDS: the RT x RT tiles of C^-1 (tile [rt][st] holds C^-1[32 rt + n][32 st + k], the B operand of
// mfma_tile_nt as it is, C^-1 being symmetric), then each wave's RT tiles of its rows of W.
__global__ __launch_bounds__(kTileThreads) void k_lowrank_entropy_rows_mfma(
    const float* __restrict__ W, const float* __restrict__ d, const float* __restrict__ cinv,
    int64_t D, int64_t R, int64_t groups, float* __restrict__ dW, float* __restrict__ dd,
    double* __restrict__ partial) {
  extern __shared__ float tiles[];
  __shared__ float invd[kTileWaves][kTile];
  __shared__ double red[kTileWaves];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int RT = (int)((R + kTile - 1) / kTile);
  float* cs = tiles;
  float* ws = tiles + (RT * RT + w * RT) * kTileFloats;
  const bool grads = dW != nullptr;
  if (grads) {
    for (int e = threadIdx.x; e < RT * RT * kTile * kTile; e += kTileThreads) {
      const int tile = e >> 10, n = (e >> 5) & 31, k = e & 31;
      const int rt = tile / RT, st = tile - rt * RT;
      const int64_t rr = (int64_t)rt * kTile + n, ss = (int64_t)st * kTile + k;
      cs[tile * kTileFloats + n * kTileStride + k] = (rr < R && ss < R) ? cinv[rr * R + ss] : 0.0f;
    }
  }
  __syncthreads();
  double logs = 0.0;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {   // (block-uniform bounds)
    const int64_t ibase = (g * kTileWaves + w) * kTile;
    const bool active = ibase < D;
    if (active && half == 0) {
      const int64_t i = ibase + col;
      const float di = i < D ? d[i] : 1.0f;
      if (i < D) logs += log((double)di);
      invd[w][col] = 1.0f / di;
    }
    if (active && grads) {
      for (int st = 0; st < RT; ++st) {
        const int64_t r = (int64_t)st * kTile + col;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t ii = ibase + 2 * q + half;
          ws[st * kTileFloats + (2 * q + half) * kTileStride + col] =
              (ii < D && r < R) ? W[ii * R + r] : 0.0f;
        }
      }
    }
    __syncthreads();
    float p[16];   // this lane's 16 rows of sum_r M[i, r] W[i, r], its column of every r tile
#pragma unroll
    for (int q = 0; q < 16; ++q) p[q] = 0.0f;
    if (active && grads) {
      for (int rt = 0; rt < RT; ++rt) {
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        for (int st = 0; st < RT; ++st)   // A[row][s] = W, B[r][s] = C^-1
          mfma_tile_nt(acc, ws + st * kTileFloats, cs + (rt * RT + st) * kTileFloats, lane);
        const int64_t r = (int64_t)rt * kTile + col;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = acc_row(q, lane);
          const int64_t i = ibase + row;
          p[q] = fmaf(acc[q], ws[rt * kTileFloats + row * kTileStride + col], p[q]);
          if (i < D && r < R) dW[i * R + r] = acc[q] * invd[w][row];
        }
      }
    }
    __syncthreads();   // the wave's tiles of W are read: tile 0 now takes p
    if (active && grads) {
#pragma unroll
      for (int q = 0; q < 16; ++q) ws[acc_row(q, lane) * kTileStride + col] = p[q];
    }
    __syncthreads();
    if (active && grads && half == 0) {
      const int64_t i = ibase + col;
      float q = 0.0f;
#pragma unroll
      for (int c = 0; c < kTile; ++c) q += ws[col * kTileStride + c];
      const float inv = invd[w][col];
      if (i < D) dd[i] = 0.5f * (inv - q * inv * inv);
    }
    __syncthreads();
  }
  block_sum_to<kTileThreads>(logs, red, partial);
}

// ---- 3. the finish -----------------------------------------------------------------------------
// thread t sums partials [t per, (t + 1) per) in order, then the threads in a fixed tree
__global__ __launch_bounds__(kLeSumThreads) void k_lowrank_entropy_finish(
    const double* __restrict__ partial, int64_t n, const double* __restrict__ logdet, int64_t D,
    float* __restrict__ entropy) {
  __shared__ double red[kLeSumThreads / kWave];
  const int64_t per = (n + kLeSumThreads - 1) / kLeSumThreads;
  const int64_t q0 = threadIdx.x * per, q1 = min(n, q0 + per);
  double s = 0.0;
  for (int64_t q = q0; q < q1; ++q) s += partial[q];
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double logd = 0.0;
    for (int q = 0; q < kLeSumThreads / kWave; ++q) logd += red[q];
    *entropy = (float)(0.5 * (double)D * (1.0 + log(2.0 * M_PI)) + *logdet + 0.5 * logd);
  }
}

}  // namespace mi

namespace {

constexpr int64_t kFill = 1024;            // blocks that fill the chip (256 CUs, a few each)
constexpr size_t kStaticLds = 64 * 1024;   // what a launch may ask for without saying so first

struct LeGeometry {
  bool mfma;
  int64_t units;    // tiles of 256 rows (VALU) or groups of four tiles of 32 rows (MFMA)
  int64_t blocks;   // each walks units b, b + blocks, ...
};

LeGeometry le_geometry(int64_t D, int64_t R) {
  LeGeometry g{};
  g.mfma = R >= mi::kTile;
  g.units = g.mfma ? ceil_div(D, (int64_t)mi::kTile * mi::kTileWaves)
                   : ceil_div(D, mi::kLeRowThreads);
  g.blocks = std::min<int64_t>(g.units, kFill);
  return g;
}

int le_check_shape(int64_t D, int64_t R) {
  if (D < 1 || R < 1) return MI_EINVAL;
  if (D > MI_LOWRANK_MAX_D || R > MI_LOWRANK_MAX_R) return MI_EUNSUPPORTED;
  return 0;
}

// workspace: C^-1 (R R floats, padded to 8 bytes), sum_j log L[j, j], the blocks' partials
size_t le_cinv_bytes(int64_t R) { return ((size_t)(R * R) * sizeof(float) + 7) & ~(size_t)7; }

// a launch with more dynamic LDS than the default limit says so first
template <typename Kernel>
hipError_t le_allow_lds(Kernel kernel, size_t bytes) {
  if (bytes <= kStaticLds) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

int valu_quads(int64_t R) { return R <= 4 ? 1 : R <= 8 ? 2 : R <= 16 ? 4 : 8; }

}  // namespace

extern "C" {

int mi_lowrank_entropy_workspace_bytes(int64_t D, int64_t R, size_t* bytes) {
  const int bad = le_check_shape(D, R);
  if (bad != 0) return bad;
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = le_cinv_bytes(R) + sizeof(double) * (size_t)(1 + le_geometry(D, R).blocks);
  return 0;
}

int mi_lowrank_entropy(const float* cov_factor, const float* cov_diag,
                       const float* capacitance_tril, int64_t D, int64_t R, void* workspace,
                       size_t workspace_bytes, float* entropy, float* dcov_factor,
                       float* dcov_diag, void* stream) {
  const int bad = le_check_shape(D, R);
  if (bad != 0) return bad;
  if (cov_factor == nullptr || cov_diag == nullptr || capacitance_tril == nullptr ||
      entropy == nullptr || (dcov_factor == nullptr) != (dcov_diag == nullptr))
    return MI_EINVAL;
  size_t need = 0;
  mi_lowrank_entropy_workspace_bytes(D, R, &need);
  if (workspace == nullptr || workspace_bytes < need) return MI_EINVAL;
  const LeGeometry g = le_geometry(D, R);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int grads = dcov_factor != nullptr;
  float* cinv = static_cast<float*>(workspace);
  double* logdet = reinterpret_cast<double*>(static_cast<char*>(workspace) + le_cinv_bytes(R));
  double* partial = logdet + 1;

  const int n = (int)R;
  const size_t lds1 = sizeof(double) * (size_t)(n * (n | 1) + n);
  hipError_t e = le_allow_lds(mi::k_lowrank_entropy_capacitance, lds1);
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_lowrank_entropy_capacitance, dim3(1), dim3(n <= 32 ? 256 : 1024), lds1,
                     s, capacitance_tril, n, grads, cinv, logdet);
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);

  const dim3 grid((unsigned)g.blocks);
  if (g.mfma) {
    const int64_t RT = ceil_div(R, mi::kTile);
    const size_t lds2 = sizeof(float) * (size_t)((RT * RT + mi::kTileWaves * RT) * mi::kTileFloats);
    e = le_allow_lds(mi::k_lowrank_entropy_rows_mfma, lds2);
    if (e != hipSuccess) return to_code(e);
    hipLaunchKernelGGL(mi::k_lowrank_entropy_rows_mfma, grid, dim3(mi::kTileThreads), lds2, s,
                       cov_factor, cov_diag, cinv, D, R, g.units, dcov_factor, dcov_diag, partial);
  } else {
#define MI_LE_ROWS(RQ)                                                                          \
  hipLaunchKernelGGL(mi::k_lowrank_entropy_rows_valu<RQ>, grid, dim3(mi::kLeRowThreads), 0, s,  \
                     cov_factor, cov_diag, cinv, D, R, g.units, dcov_factor, dcov_diag, partial)
    switch (valu_quads(R)) {
      case 1: MI_LE_ROWS(1); break;
      case 2: MI_LE_ROWS(2); break;
      case 4: MI_LE_ROWS(4); break;
      default: MI_LE_ROWS(8); break;
    }
#undef MI_LE_ROWS
  }
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_lowrank_entropy_finish, dim3(1), dim3(mi::kLeSumThreads), 0, s, partial,
                     g.blocks, logdet, D, entropy);
  return to_code(hipGetLastError());
}

}  // extern "C"
