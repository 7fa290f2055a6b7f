// Reparameterised draws of a full-covariance MultivariateNormal guide factor and their backward.
//
// Replaces MultivariateNormal.rsample (torch multivariate_normal.py:247-250: loc + L eps through
// _batch_mv) over K particles, and the gradients autograd computes through it:
//   z[k, i]  = loc[i] + sum_{j <= i} L[i, j] eps[k, j]
//   dloc[i]  = sum_k dz[k, i]
//   dL[i, j] = sum_k dz[k, i] eps[k, j]   (j <= i; 0 above the diagonal)
// eps[k, j] is the Philox normal of (seed, step, stream, global particle, element j) that
// mi_normal_rsample draws with N = D. It lives in LDS and registers only: the backward regenerates
// it from the counter.
//
// D >= 32: both products run on v_mfma_f32_32x32x2_f32 over 32 x 32 tiles, lower-triangular tile
// pairs only, the diagonal tile masked per element while it is staged.
//   forward  Z[k, i]  (A = eps[k, j], B = L[i, j]): a block is one tile of 32 particles and four
//            element tiles (one per wave); the eps tile of each j step is generated once per block.
//   backward DL[i, j] (A = dz[k, i], B = eps[k, j]): a block is one j tile, four i tiles (one per
//            wave) and one slice of the particle tiles; slices are combined in a fixed order.
// Every z[k, i] is the chain acc = loc[i]; acc = fma(eps[k, j], L[i, j], acc) for j ascending (an
// f32 MFMA is exactly that chain), whichever tile row the particle falls in: a draw does not depend
// on particle_offset or on K. D < 32 runs the same chain on the VALU.
#include "internal.hpp"
#include "mfma_tile.hpp"

#include <algorithm>

namespace mi {

constexpr int kMvnThreads = 256;   // the VALU kernels and the slice combination

// ---- forward, D >= 32 ------------------------------------------------------------------------
__global__ __launch_bounds__(kTileThreads) void k_mvn_rsample_mfma(
    const float* __restrict__ loc, const float* __restrict__ L, int64_t K, int64_t D,
    uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev, uint32_t stream_id,
    int64_t poff, const float* __restrict__ eps_in, float* __restrict__ z) {
  __shared__ float es[kTileFloats];
  __shared__ float ls[kTileWaves][kTileFloats];
  if (step_dev != nullptr) step += *step_dev;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int T = (int)((D + kTile - 1) / kTile);
  // the longest chains (the last element tiles) start first
  const int group = (int)(gridDim.y - 1 - blockIdx.y);
  const int it = group * kTileWaves + w;
  const bool active = it < T;
  const int jt_last = min(T - 1, group * kTileWaves + kTileWaves - 1);
  const int64_t kbase = (int64_t)blockIdx.x * kTile;
  const int64_t ibase = (int64_t)it * kTile;
  const NormalsKey key{seed, step, stream_id, poff, eps_in, D};
  const NormalsSection sec{D, 0, 0};   // eps: the whole stream of the factor

  // L[ibase + 2 r + half, 32 jt + col] for r = 0 .. 15, zero above the diagonal and outside D
  // (the strict upper triangle is never read)
  float lreg[16];
  auto load_l = [&](int jt) {
    const int64_t j = (int64_t)jt * kTile + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t i = ibase + 2 * r + half;
      lreg[r] = (i < D && j <= i) ? L[i * D + j] : 0.0f;
    }
  };
  f32x16 acc;
  {
    const int64_t i = ibase + col;
    const float m = (active && i < D) ? loc[i] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = m;
  }
  if (active) load_l(0);
  for (int jt = 0; jt <= jt_last; ++jt) {
    const bool mine = active && jt <= it;
    if (mine) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ls[w][(2 * r + half) * kTileStride + col] = lreg[r];
    }
    stage_tile<kTileThreads>(es, key, sec, kbase, K, (int64_t)jt * kTile, threadIdx.x);
    __syncthreads();
    if (active && jt + 1 <= it) load_l(jt + 1);   // in flight behind the MFMAs
    if (mine) mfma_tile_nt(acc, es, ls[w], lane);   // A[particle][j], B[j][i] = L[i][j]
    __syncthreads();
  }
  if (!active) return;
  const int64_t i = ibase + col;
  if (i >= D) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t k = kbase + acc_row(r, lane);
    if (k < K) z[k * D + i] = acc[r];
  }
}

// ---- forward, D < 32: the same chain, one thread per draw element --------------------------------
__global__ __launch_bounds__(kMvnThreads) void k_mvn_rsample_valu(
    const float* __restrict__ loc, const float* __restrict__ L, int64_t K, int64_t D,
    uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev, uint32_t stream_id,
    int64_t poff, const float* __restrict__ eps_in, float* __restrict__ z) {
  if (step_dev != nullptr) step += *step_dev;
  const int64_t t = (int64_t)blockIdx.x * kMvnThreads + threadIdx.x;
  if (t >= K * D) return;
  const int64_t k = t / D, i = t - k * D;
  float acc = loc[i];
  for (int64_t j0 = 0; j0 <= i; j0 += 4) {
    float e[4];
    if (eps_in != nullptr) {
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c] = (j0 + c <= i) ? eps_in[k * D + j0 + c] : 0.0f;
    } else {
      guide_normals(seed, step, stream_id, (uint64_t)(j0 >> 2), (uint64_t)(poff + k), e);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (j0 + c <= i) acc = fmaf(e[c], L[i * D + j0 + c], acc);
  }
  z[t] = acc;
}

// ---- backward, D >= 32 -----------------------------------------------------------------------
// grid (j tile, group of four i tiles, particle slice). out_l / out_loc: the outputs themselves
// (one slice) or this slice's [D * D] / [D] partials.
__global__ __launch_bounds__(kTileThreads) void k_mvn_rsample_bwd_mfma(
    const float* __restrict__ dz, int64_t dz_sk, int64_t dz_si, int64_t K, int64_t D,
    uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev, uint32_t stream_id,
    int64_t poff, const float* __restrict__ eps_in, int tiles_per_slice, int64_t slice_stride,
    float* __restrict__ out_loc, float* __restrict__ out_l) {
  __shared__ float es[kTileFloats];
  __shared__ float ds[kTileWaves][kTileFloats];
  if (step_dev != nullptr) step += *step_dev;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int T = (int)((D + kTile - 1) / kTile);
  const int jt = blockIdx.x;
  const int it = (int)blockIdx.y * kTileWaves + w;
  const bool single = gridDim.z == 1;
  const int64_t ibase = (int64_t)it * kTile, jbase = (int64_t)jt * kTile;
  float* __restrict__ dst_l = out_l + (int64_t)blockIdx.z * slice_stride;
  float* __restrict__ dst_loc = out_loc + (int64_t)blockIdx.z * D;
  const bool lower = it < T && jt <= it;   // this wave's tile holds entries of the lower triangle
  // no wave of the block has such a tile: nothing to sum (block-uniform)
  const bool any_lower = (int)blockIdx.y * kTileWaves + kTileWaves - 1 >= jt;
  const NormalsKey key{seed, step, stream_id, poff, eps_in, D};
  const NormalsSection sec{D, 0, 0};   // eps: the whole stream of the factor
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float sum_loc = 0.0f;
  if (any_lower) {
    const int64_t nkt = (K + kTile - 1) / kTile;
    const int64_t kt0 = (int64_t)blockIdx.z * tiles_per_slice;
    const int64_t kt1 = min(nkt, kt0 + tiles_per_slice);
    for (int64_t kt = kt0; kt < kt1; ++kt) {
      const int64_t kbase = kt * kTile;
      if (lower) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stage_dz_row(ds[w], dz, dz_sk, dz_si, kbase, K, ibase, D, r, lane);
      }
      stage_tile<kTileThreads>(es, key, sec, kbase, K, jbase, threadIdx.x);
      __syncthreads();
      if (lower) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float a = tile_k_major(ds[w], s, lane);   // A[i][k] = dz[k][i]
          const float b = tile_k_major(es, s, lane);      // B[k][j] = eps[k][j]
          sum_loc += a;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  if (it >= T) return;
  if (!lower && !single) return;   // the slices' combination writes the zeros
  const int64_t j = jbase + col;
  if (j < D) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t i = ibase + acc_row(r, lane);
      if (i < D) dst_l[i * D + j] = (lower && j <= i) ? acc[r] : 0.0f;
    }
  }
  if (jt == 0) {   // (lower for every i tile) even plus odd particles of each element
    const float total = sum_loc + __shfl_xor(sum_loc, 32, kWave);
    const int64_t i = ibase + col;
    if (half == 0 && i < D) dst_loc[i] = total;
  }
}

// ---- backward, D < 32: one thread per entry of the lower triangle and particle slice ---------
__global__ __launch_bounds__(kMvnThreads) void k_mvn_rsample_bwd_valu(
    const float* __restrict__ dz, int64_t dz_sk, int64_t dz_si, int64_t K, int64_t D,
    uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev, uint32_t stream_id,
    int64_t poff, const float* __restrict__ eps_in, int64_t rows_per_slice, int64_t slice_stride,
    float* __restrict__ out_loc, float* __restrict__ out_l) {
  if (step_dev != nullptr) step += *step_dev;
  const int64_t t = (int64_t)blockIdx.x * kMvnThreads + threadIdx.x;
  if (t >= D * D) return;
  const int64_t i = t / D, j = t - i * D;
  float* __restrict__ dst_l = out_l + (int64_t)blockIdx.y * slice_stride;
  float* __restrict__ dst_loc = out_loc + (int64_t)blockIdx.y * D;
  if (j > i) {
    dst_l[t] = 0.0f;
    return;
  }
  const int64_t k0 = (int64_t)blockIdx.y * rows_per_slice;
  const int64_t k1 = min(K, k0 + rows_per_slice);
  float acc = 0.0f, sum_loc = 0.0f;
  for (int64_t k = k0; k < k1; ++k) {
    const float g = dz[k * dz_sk + i * dz_si];
    float e;
    if (eps_in != nullptr) {
      e = eps_in[k * D + j];
    } else {
      float quad[4];
      guide_normals(seed, step, stream_id, (uint64_t)(j >> 2), (uint64_t)(poff + k), quad);
      const int c = (int)(j & 3);
      e = c == 0 ? quad[0] : c == 1 ? quad[1] : c == 2 ? quad[2] : quad[3];
    }
    sum_loc += g;
    acc = fmaf(g, e, acc);
  }
  dst_l[t] = acc;
  if (j == 0) dst_loc[i] = sum_loc;
}

// Sum the slices' partials in a fixed order (fp64): the lower triangle of dL (zeros above it) and
// dloc.
__global__ __launch_bounds__(kMvnThreads) void k_mvn_sum_slices(const float* __restrict__ part_l,
                                                                const float* __restrict__ part_loc,
                                                                int64_t slices, int64_t D,
                                                                float* __restrict__ dloc,
                                                                float* __restrict__ dl) {
  const int64_t t = (int64_t)blockIdx.x * kMvnThreads + threadIdx.x;
  const int64_t n = D * D;
  if (t < n) {
    const int64_t i = t / D, j = t - i * D;
    double s = 0.0;
    if (j <= i)
      for (int64_t q = 0; q < slices; ++q) s += (double)part_l[q * n + t];
    dl[t] = (float)s;
  }
  if (t < D) {
    double s = 0.0;
    for (int64_t q = 0; q < slices; ++q) s += (double)part_loc[q * D + t];
    dloc[t] = (float)s;
  }
}

}  // namespace mi

namespace {

int check_shape(int64_t K, int64_t D) {
  if (K < 1 || D < 1) return MI_EINVAL;
  if (D > MI_MVN_MAX_N) return MI_EUNSUPPORTED;
  return 0;
}

// Particle slices of the backward: enough blocks to fill the chip, whole particle tiles (MFMA) or
// at least 64 particles (VALU) per slice.
struct MvnBwdGeometry {
  bool mfma;
  int64_t tiles;     // element tiles per axis (MFMA)
  int64_t per;       // particle tiles (MFMA) or particles (VALU) per slice
  int64_t slices;
};

MvnBwdGeometry mvn_bwd_geometry(int64_t K, int64_t D) {
  MvnBwdGeometry g{};
  g.mfma = D >= mi::kTile;
  if (g.mfma) {
    g.tiles = ceil_div(D, mi::kTile);
    const int64_t lower = g.tiles * (g.tiles + 1) / 2;
    const int64_t nkt = ceil_div(K, mi::kTile);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(nkt, ceil_div(512, lower)));
    g.per = ceil_div(nkt, want);
    g.slices = ceil_div(nkt, g.per);
  } else {
    g.per = std::max<int64_t>(64, ceil_div(K, 256));
    g.slices = ceil_div(K, g.per);
  }
  return g;
}

}  // namespace

extern "C" {

int mi_mvn_rsample(const float* loc, const float* scale_tril, int64_t K, int64_t D, uint64_t seed,
                   uint64_t step, const uint64_t* step_device, uint32_t stream_id,
                   int64_t particle_offset, const float* eps, float* z, void* stream) {
  const int bad = check_shape(K, D);
  if (bad != 0) return bad;
  if (loc == nullptr || scale_tril == nullptr || z == nullptr || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (D >= mi::kTile) {
    const dim3 grid((unsigned)ceil_div(K, mi::kTile),
                    (unsigned)ceil_div(ceil_div(D, mi::kTile), mi::kTileWaves));
    hipLaunchKernelGGL(mi::k_mvn_rsample_mfma, grid, dim3(mi::kTileThreads), 0, s, loc, scale_tril,
                       K, D, seed, step, step_device, stream_id, particle_offset, eps, z);
  } else {
    hipLaunchKernelGGL(mi::k_mvn_rsample_valu, dim3((unsigned)ceil_div(K * D, mi::kMvnThreads)),
                       dim3(mi::kMvnThreads), 0, s, loc, scale_tril, K, D, seed, step, step_device,
                       stream_id, particle_offset, eps, z);
  }
  return to_code(hipGetLastError());
}

int mi_mvn_rsample_backward_workspace_bytes(int64_t K, int64_t D, size_t* bytes) {
  const int bad = check_shape(K, D);
  if (bad != 0) return bad;
  if (bytes == nullptr) return MI_EINVAL;
  const MvnBwdGeometry g = mvn_bwd_geometry(K, D);
  *bytes = g.slices > 1 ? (size_t)g.slices * (size_t)(D * D + D) * sizeof(float) : 0;
  return 0;
}

int mi_mvn_rsample_backward(const float* dz, int64_t dz_stride_k, int64_t dz_stride_i, int64_t K,
                            int64_t D, uint64_t seed, uint64_t step, const uint64_t* step_device,
                            uint32_t stream_id, int64_t particle_offset, const float* eps,
                            void* workspace, size_t workspace_bytes, float* dloc,
                            float* dscale_tril, void* stream) {
  const int bad = check_shape(K, D);
  if (bad != 0) return bad;
  if (dz == nullptr || dloc == nullptr || dscale_tril == nullptr || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  size_t need = 0;
  mi_mvn_rsample_backward_workspace_bytes(K, D, &need);
  if (!workspace_ok(workspace, workspace_bytes, need)) return MI_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MvnBwdGeometry g = mvn_bwd_geometry(K, D);
  float* out_l = slice_out(dscale_tril, workspace, g.slices, 0);
  float* out_loc = slice_out(dloc, workspace, g.slices, g.slices * D * D);
  if (g.mfma) {
    const dim3 grid((unsigned)g.tiles, (unsigned)ceil_div(g.tiles, mi::kTileWaves),
                    (unsigned)g.slices);
    hipLaunchKernelGGL(mi::k_mvn_rsample_bwd_mfma, grid, dim3(mi::kTileThreads), 0, s, dz,
                       dz_stride_k, dz_stride_i, K, D, seed, step, step_device, stream_id,
                       particle_offset, eps, (int)g.per, D * D, out_loc, out_l);
  } else {
    const dim3 grid((unsigned)ceil_div(D * D, mi::kMvnThreads), (unsigned)g.slices);
    hipLaunchKernelGGL(mi::k_mvn_rsample_bwd_valu, grid, dim3(mi::kMvnThreads), 0, s, dz,
                       dz_stride_k, dz_stride_i, K, D, seed, step, step_device, stream_id,
                       particle_offset, eps, g.per, D * D, out_loc, out_l);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || g.slices == 1) return to_code(e);
  const int64_t threads = std::max<int64_t>(D * D, D);
  hipLaunchKernelGGL(mi::k_mvn_sum_slices, dim3((unsigned)ceil_div(threads, mi::kMvnThreads)),
                     dim3(mi::kMvnThreads), 0, s, out_l, out_loc, g.slices, D, dloc, dscale_tril);
  return to_code(hipGetLastError());
}

}  // extern "C"
