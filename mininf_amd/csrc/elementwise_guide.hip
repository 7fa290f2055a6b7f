// Guide factors of the one-noise-word families: Exponential, Laplace, Cauchy, HalfCauchy,
// HalfNormal and LogNormal.
//
// Replaces FactorizedDistribution.rsample (mininf/nn.py:133-145) for those families, i.e. torch's
// Exponential.rsample (exponential.py:69-71), Laplace.rsample (laplace.py:74-88), Cauchy.rsample
// (cauchy.py:77-80) and the TransformedDistribution.rsample of HalfCauchy, HalfNormal and
// LogNormal, the gradients autograd computes through them, and their entropy() with its autograd.
//
// The transform is the predictive sites' (elementwise_draw.hpp pred_draw), the counter the Normal
// factor's: element i of particle k takes word i % 4 of guide_bits(seed, step, stream_id, sub 0,
// quad i / 4, particle_offset + k). Draws are row-major z[k, i]. The noise is never stored: the
// backward regenerates it from the counter.
#include "elementwise_draw.hpp"
#include "internal.hpp"

namespace mi {

constexpr int kElemThreads = 256;

// The quad's four noise words: uniforms, or the Normal factor's eps for the normal-based families.
template <int FAMILY>
MI_DEV void elementwise_noise(uint64_t seed, uint64_t step, uint32_t stream_id, int64_t quad,
                              int64_t particle, float v[4]) {
  if (pred_normal_based(FAMILY)) {
    guide_normals(seed, step, stream_id, (uint64_t)quad, (uint64_t)particle, v);
  } else {
    const U4 w = guide_bits(seed, step, stream_id, 0, (uint64_t)quad, (uint64_t)particle);
    v[0] = u01(w.x);
    v[1] = u01(w.y);
    v[2] = u01(w.z);
    v[3] = u01(w.w);
  }
}

// One thread per (particle, element quad): flat t = k * quads + quad.
template <int FAMILY>
__global__ __launch_bounds__(kElemThreads) void k_elementwise_rsample(
    const float* __restrict__ a, int64_t a_s, const float* __restrict__ b, int64_t b_s, int64_t K,
    int64_t N, int64_t quads, uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev,
    uint32_t stream_id, int64_t poff, const float* __restrict__ noise, float* __restrict__ z) {
  const int64_t t = (int64_t)blockIdx.x * kElemThreads + threadIdx.x;
  if (t >= K * quads) return;
  const int64_t k = t / quads, quad = t - k * quads;
  const int64_t i0 = quad * 4;
  float v[4];
  if (noise != nullptr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i0 + j < N) ? noise[k * N + i0 + j] : 0.5f;
  } else {
    if (step_dev != nullptr) step += *step_dev;
    elementwise_noise<FAMILY>(seed, step, stream_id, quad, poff + k, v);
  }
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = min(i0 + j, N - 1);
    const float av = a[i * a_s];
    const float bv = pred_two_parameters(FAMILY) ? b[i * b_s] : 0.0f;
    o[j] = pred_draw<FAMILY>(av, bv, guide_noise<FAMILY>(v[j]));
  }
  float* row = z + k * N + i0;
  if (i0 + 4 <= N && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
    *reinterpret_cast<float4*>(row) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < N) row[j] = o[j];
  }
}

// Backward of the draw, reduced over particles: the geometry of k_normal_rsample_bwd (guide.hip),
// ti quad lanes x 256 / ti particle lanes per block, one particle slice per blockIdx.y. A thread
// sums its particles in fp64 in ascending order; the particle lanes meet in LDS in lane order.
// out_a / out_b: the outputs themselves (one slice) or the per-slice partials [slices, N].
template <int FAMILY>
__global__ __launch_bounds__(kElemThreads) void k_elementwise_rsample_bwd(
    const float* __restrict__ dz, int64_t dz_sk, int64_t dz_si, const float* __restrict__ a,
    int64_t a_s, const float* __restrict__ b, int64_t b_s, int64_t K, int64_t N, uint64_t seed,
    uint64_t step, const uint64_t* __restrict__ step_dev, uint32_t stream_id, int64_t poff,
    const float* __restrict__ noise, float* __restrict__ out_a, float* __restrict__ out_b,
    int64_t rows_per_block, int ti) {
  constexpr bool kTwo = pred_two_parameters(FAMILY);
  __shared__ double red[kElemThreads][kTwo ? 8 : 4];
  if (step_dev != nullptr) step += *step_dev;
  const int tx = threadIdx.x % ti, ty = threadIdx.x / ti, tk = kElemThreads / ti;
  const int64_t quad = (int64_t)blockIdx.x * ti + tx;
  const int64_t i0 = quad * 4;
  const int64_t k0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t k1 = min(K, k0 + rows_per_block);
  double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
  if (i0 < N) {
    float av[4], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = min(i0 + j, N - 1);
      av[j] = a[i * a_s];
      bv[j] = kTwo ? b[i * b_s] : 0.0f;
    }
    for (int64_t k = k0 + ty; k < k1; k += tk) {
      const float* row = dz + k * dz_sk + i0 * dz_si;
      float g[4];
      if (dz_si == 1 && i0 + 4 <= N && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(row);
        g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = (i0 + j < N) ? row[j * dz_si] : 0.0f;
      }
      float v[4];
      if (noise != nullptr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (i0 + j < N) ? noise[k * N + i0 + j] : 0.5f;
      } else {
        elementwise_noise<FAMILY>(seed, step, stream_id, quad, poff + k, v);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float fa, fb;
        guide_draw_factors<FAMILY>(av[j], bv[j], guide_noise<FAMILY>(v[j]), fa, fb);
        sa[j] = fma((double)g[j], (double)fa, sa[j]);
        if (kTwo) sb[j] = fma((double)g[j], (double)fb, sb[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[threadIdx.x][j] = sa[j];
    if (kTwo) red[threadIdx.x][4 + j] = sb[j];
  }
  __syncthreads();
  if (ty == 0 && i0 < N) {
    double ta[4] = {0.0, 0.0, 0.0, 0.0}, tb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < tk; ++r) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ta[j] += red[r * ti + tx][j];
        if (kTwo) tb[j] += red[r * ti + tx][4 + j];
      }
    }
    const int64_t base = (int64_t)blockIdx.y * N + i0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < N) {
        if (out_a != nullptr) out_a[base + j] = (float)ta[j];
        if (kTwo && out_b != nullptr) out_b[base + j] = (float)tb[j];
      }
    }
  }
}

// Sum the `slices` rows of up to two [slices, N] partial arrays (fixed order, fp64).
__global__ __launch_bounds__(kElemThreads) void k_elementwise_sum_slices(
    const float* __restrict__ part_a, const float* __restrict__ part_b, int64_t slices, int64_t N,
    float* __restrict__ out_a, float* __restrict__ out_b) {
  const int64_t i = (int64_t)blockIdx.x * kElemThreads + threadIdx.x;
  if (i >= N) return;
  if (out_a != nullptr) {
    double s = 0.0;
    for (int64_t r = 0; r < slices; ++r) s += (double)part_a[r * N + i];
    out_a[i] = (float)s;
  }
  if (out_b != nullptr) {
    double s = 0.0;
    for (int64_t r = 0; r < slices; ++r) s += (double)part_b[r * N + i];
    out_b[i] = (float)s;
  }
}

// Entropy summed over the elements, and its gradient, as torch's entropy() of each class:
//   LogNormal    1/2 + 1/2 log(2 pi) + log(scale) + loc   (log_normal.py:75-76, normal.py:115-116)
//   Laplace      1 + log(2 scale)                         (laplace.py:104-105)
//   Cauchy       log(4 pi) + log(scale)                   (cauchy.py:99-100)
//   HalfCauchy   log(4 pi) + log(scale) - log(2)          (half_cauchy.py:92-93)
//   HalfNormal   1/2 + 1/2 log(2 pi) + log(scale) - log(2)  (half_normal.py:84-85)
//   Exponential  1 - log(rate)                            (exponential.py:86-87)
// One block of 1024 threads (one launch, no atomics): a thread sums the elements t, t + 1024, ...
// in fp64, and the threads' sums meet in a halving tree in LDS, so the order is a function of N
// alone. The logarithm itself is fp32 (logf, about 1 ulp): in fp64 it made this one block the
// longest launch of a step at N = 65536.
constexpr int kEntropyThreads = 1024;

template <int FAMILY>
__global__ __launch_bounds__(kEntropyThreads) void k_elementwise_entropy(
    const float* __restrict__ a, int64_t a_s, const float* __restrict__ b, int64_t b_s, int64_t N,
    float* __restrict__ H, float* __restrict__ da, float* __restrict__ db) {
  constexpr bool kTwo = pred_two_parameters(FAMILY);
  constexpr double kLogPi = 1.1447298858494001741434;
  constexpr double kLog2 = 0.6931471805599453094172;
  constexpr double kConstant =
      FAMILY == MI_PRED_LOG_NORMAL ? 0.5 + 0.5 * (kLog2 + kLogPi) :
      FAMILY == MI_PRED_LAPLACE ? 1.0 + kLog2 :
      FAMILY == MI_PRED_CAUCHY ? 2.0 * kLog2 + kLogPi :
      FAMILY == MI_PRED_HALF_CAUCHY ? kLog2 + kLogPi :
      FAMILY == MI_PRED_HALF_NORMAL ? 0.5 + 0.5 * (kLogPi - kLog2) : 1.0;
  __shared__ double red[kEntropyThreads];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += kEntropyThreads) {
    const float spread = kTwo ? b[i * b_s] : a[i * a_s];   // the scale, or the Exponential's rate
    const double l = (double)logf(spread);
    double h = kConstant + (FAMILY == MI_PRED_EXPONENTIAL ? -l : l);
    if (FAMILY == MI_PRED_LOG_NORMAL) h += (double)a[i * a_s];
    acc += h;
    const float inverse = FAMILY == MI_PRED_EXPONENTIAL ? -1.0f / spread : 1.0f / spread;
    if (kTwo) {
      if (da != nullptr) da[i] = FAMILY == MI_PRED_LOG_NORMAL ? 1.0f : 0.0f;
      if (db != nullptr) db[i] = inverse;
    } else if (da != nullptr) {
      da[i] = inverse;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int width = kEntropyThreads / 2; width > 0; width >>= 1) {
    if ((int)threadIdx.x < width) red[threadIdx.x] += red[threadIdx.x + width];
    __syncthreads();
  }
  if (threadIdx.x == 0) H[0] = (float)red[0];
}

}  // namespace mi

namespace {

constexpr int64_t kMaxElements = (int64_t)1 << 34;   // 32-bit quad counter

bool guide_family(int family) {
  return family >= MI_PRED_EXPONENTIAL && family <= MI_PRED_LOG_NORMAL;
}

// FAMILY as a template argument of `call`.
#define MI_ELEMENTWISE_DISPATCH(family, call)                                   \
  switch (family) {                                                             \
    case MI_PRED_EXPONENTIAL: call(MI_PRED_EXPONENTIAL); break;                 \
    case MI_PRED_LAPLACE: call(MI_PRED_LAPLACE); break;                         \
    case MI_PRED_CAUCHY: call(MI_PRED_CAUCHY); break;                           \
    case MI_PRED_HALF_CAUCHY: call(MI_PRED_HALF_CAUCHY); break;                 \
    case MI_PRED_HALF_NORMAL: call(MI_PRED_HALF_NORMAL); break;                 \
    default: call(MI_PRED_LOG_NORMAL); break;                                   \
  }

}  // namespace

extern "C" {

int mi_elementwise_rsample(int family, const float* a, int64_t a_stride, const float* b,
                           int64_t b_stride, int64_t K, int64_t N, uint64_t seed, uint64_t step,
                           const uint64_t* step_device, uint32_t stream_id,
                           int64_t particle_offset, const float* noise, float* z, void* stream) {
  if (!guide_family(family) || a == nullptr || z == nullptr || K < 1 || N < 1 ||
      stream_id > 0xFFFFFFu || (mi::pred_two_parameters(family) && b == nullptr))
    return MI_EINVAL;
  if (N > kMaxElements) return MI_EUNSUPPORTED;
  const int64_t quads = ceil_div(N, 4);
  if (K > (kMaxGrid * (int64_t)mi::kElemThreads) / quads) return MI_EUNSUPPORTED;
  const unsigned grid = (unsigned)ceil_div(K * quads, mi::kElemThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MI_LAUNCH(F)                                                                           \
  hipLaunchKernelGGL(mi::k_elementwise_rsample<F>, dim3(grid), dim3(mi::kElemThreads), 0, s, a, \
                     a_stride, b, b_stride, K, N, quads, seed, step, step_device, stream_id,   \
                     particle_offset, noise, z)
  MI_ELEMENTWISE_DISPATCH(family, MI_LAUNCH)
#undef MI_LAUNCH
  return to_code(hipGetLastError());
}

int mi_elementwise_rsample_backward_workspace_bytes(int64_t K, int64_t N, size_t* bytes) {
  if (K < 1 || N < 1 || bytes == nullptr) return MI_EINVAL;
  const BwdGeometry geo = bwd_geometry(K, ceil_div(N, 4), mi::kElemThreads);
  *bytes = geo.slices > 1 ? (size_t)geo.slices * 2 * (size_t)N * sizeof(float) : 0;
  return 0;
}

int mi_elementwise_rsample_backward(int family, const float* dz, int64_t dz_stride_k,
                                    int64_t dz_stride_i, const float* a, int64_t a_stride,
                                    const float* b, int64_t b_stride, int64_t K, int64_t N,
                                    uint64_t seed, uint64_t step, const uint64_t* step_device,
                                    uint32_t stream_id, int64_t particle_offset,
                                    const float* noise, void* workspace, size_t workspace_bytes,
                                    float* da, float* db, void* stream) {
  if (!guide_family(family) || dz == nullptr || a == nullptr || K < 1 || N < 1 ||
      stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  const bool two = mi::pred_two_parameters(family);
  if (two && b == nullptr) return MI_EINVAL;
  if (!two) db = nullptr;
  if (da == nullptr && db == nullptr) return MI_EINVAL;
  if (N > kMaxElements) return MI_EUNSUPPORTED;
  size_t need = 0;
  mi_elementwise_rsample_backward_workspace_bytes(K, N, &need);
  if (!workspace_ok(workspace, workspace_bytes, need)) return MI_EWORKSPACE;
  const BwdGeometry geo = bwd_geometry(K, ceil_div(N, 4), mi::kElemThreads);
  if (geo.gx > kMaxGrid) return MI_EUNSUPPORTED;
  const int64_t gy = geo.slices;
  float* out_a = da == nullptr ? nullptr : slice_out(da, workspace, gy, 0);
  float* out_b = db == nullptr ? nullptr : slice_out(db, workspace, gy, gy * N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)geo.gx, (unsigned)gy);
#define MI_LAUNCH(F)                                                                            \
  hipLaunchKernelGGL(mi::k_elementwise_rsample_bwd<F>, grid, dim3(mi::kElemThreads), 0, s, dz,  \
                     dz_stride_k, dz_stride_i, a, a_stride, b, b_stride, K, N, seed, step,      \
                     step_device, stream_id, particle_offset, noise, out_a, out_b, geo.rows,    \
                     geo.ti)
  MI_ELEMENTWISE_DISPATCH(family, MI_LAUNCH)
#undef MI_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || gy == 1) return to_code(e);
  hipLaunchKernelGGL(mi::k_elementwise_sum_slices, dim3((unsigned)ceil_div(N, mi::kElemThreads)),
                     dim3(mi::kElemThreads), 0, s, out_a, out_b, gy, N, da, db);
  return to_code(hipGetLastError());
}

int mi_elementwise_entropy(int family, const float* a, int64_t a_stride, const float* b,
                           int64_t b_stride, int64_t N, float* H, float* da, float* db,
                           void* stream) {
  if (!guide_family(family) || a == nullptr || H == nullptr || N < 1 ||
      (mi::pred_two_parameters(family) && b == nullptr))
    return MI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MI_LAUNCH(F)                                                                          \
  hipLaunchKernelGGL(mi::k_elementwise_entropy<F>, dim3(1), dim3(mi::kEntropyThreads), 0, s, a, \
                     a_stride, b, b_stride, N, H, da, db)
  MI_ELEMENTWISE_DISPATCH(family, MI_LAUNCH)
#undef MI_LAUNCH
  return to_code(hipGetLastError());
}

}  // extern "C"
