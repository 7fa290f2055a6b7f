// The fixed-order fp64 reductions the site launches share: the finalize of per-(segment, particle)
// partials (sites.hip, bcast_site.hip and linear.hip write them; elbo.hip takes the same jobs as
// mi_reduce when it fuses the reduction), the sum of a fused draw's per-K-block partials, and the
// backward rescale of speculative dense gradients that every autograd node calls. Results are
// deterministic run to run. Host interface: internal.hpp.
#include "common.hpp"
#include "internal.hpp"
namespace mi {

// -------------------------------------------------------------------------------------------------
// Finalize: fixed-order fp64 reduction of partials over segments.
// -------------------------------------------------------------------------------------------------
struct FinalizeArgs {
  int32_t num_sites;
  int32_t num_slots;
  int32_t rank1;      // bit v: value v in the rank-one layout (mi_reduce.rank1)
  int32_t ksum;       // bit v: site value v is particle-summed (mi_reduce.ksum): no block, skipped
  double scale[MI_MAX_SITES];  // num_sites <= MI_MAX_SITES
  double slot_scale;  // the group's grad_scale: slot gradients are speculative like dense ones
};

// One block per 64 particles; its 1024 threads split the segments 16 ways (fixed assignment), each
// sums its share in fp64 with independent loads in flight, then the 16 shares are combined in a
// fixed order through LDS -- deterministic, and ~16x the memory-level parallelism of a thread-per-
// particle loop.
constexpr int kFinK = 64;
constexpr int kFinG = 16;

// Stage 1 of the two-stage finalize for long segment lists: block (k-block, v, chunk) sums the
// chunk's segments of value v for 64 particles (fixed order) into stage[v][chunk][k] (fp64).
constexpr int64_t kFinChunk = 256;

__global__ __launch_bounds__(kFinK * kFinG) void k_finalize_chunks(const float* __restrict__ part,
                                                                  int64_t nseg, int64_t K,
                                                                  double* __restrict__ stage) {
  __shared__ double red[kFinG][kFinK];
  const int kl = threadIdx.x % kFinK;
  const int gl = threadIdx.x / kFinK;
  const int64_t k = (int64_t)blockIdx.x * kFinK + kl;
  const int64_t kc = k < K ? k : K - 1;
  const int64_t v = blockIdx.y, c = blockIdx.z, nchunk = gridDim.z;
  const int64_t g0 = c * kFinChunk, g1 = min(nseg, g0 + kFinChunk);
  const float* p = part + v * nseg * K + kc;
  double a0 = 0.0, a1 = 0.0;
  int64_t g = g0 + gl;
  for (; g + kFinG < g1; g += 2 * kFinG) {
    a0 += (double)p[g * K];
    a1 += (double)p[(g + kFinG) * K];
  }
  for (; g < g1; g += kFinG) a0 += (double)p[g * K];
  red[gl][kl] = a0 + a1;
  __syncthreads();
  if (gl == 0 && k < K) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kFinG; ++j) acc += red[j][kl];
    stage[(v * nchunk + c) * K + k] = acc;
  }
}

template <typename T>
__global__ __launch_bounds__(kFinK * kFinG) void k_finalize(const T* __restrict__ part,
                                                           int64_t nseg, int64_t K,
                                                           const FinalizeArgs A,
                                                           float* __restrict__ total,
                                                           double* __restrict__ site_lp,
                                                           float* __restrict__ slot_grad) {
  __shared__ double red[kFinG][kFinK];
  const int kl = threadIdx.x % kFinK;
  const int gl = threadIdx.x / kFinK;
  const int64_t k = (int64_t)blockIdx.x * kFinK + kl;
  const int64_t kc = k < K ? k : K - 1;
  double t = 0.0;
  const int nv = A.num_sites + A.num_slots;
  // With one (combined) site value, blockIdx.y selects the value: many-slot groups (linear sites:
  // one slot per coefficient) reduce in parallel instead of one value after another.
  const bool split = gridDim.y > 1;
  const int v_begin = split ? (int)blockIdx.y : 0;
  const int v_end = split ? v_begin + 1 : nv;
  for (int v = v_begin; v < v_end; ++v) {
    const bool r1 = (A.rank1 >> v) & 1;
    if ((A.ksum >> v) & 1) continue;   // (uniform over the block)
    const int blk = v - __popc((unsigned)A.ksum & ((1u << v) - 1u));
    // rank one: the particle-independent u[seg] (stride 1) instead of the per-particle column
    const T* p = part + (int64_t)blk * nseg * K + (r1 ? 0 : kc);
    const int64_t stride = r1 ? 1 : K;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t g = gl;
    for (; g + 3 * kFinG < nseg; g += 4 * kFinG) {
      a0 += (double)p[g * stride];
      a1 += (double)p[(g + kFinG) * stride];
      a2 += (double)p[(g + 2 * kFinG) * stride];
      a3 += (double)p[(g + 3 * kFinG) * stride];
    }
    for (; g < nseg; g += kFinG) a0 += (double)p[g * stride];
    __syncthreads();
    red[gl][kl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (gl == 0 && k < K) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kFinG; ++j) acc += red[j][kl];
      if (r1) {
        const T* q = part + (int64_t)blk * nseg * K + nseg;
        acc = (double)q[kc] * acc + (double)q[K + kc];
      }
      if (v < A.num_sites) {
        acc *= A.scale[v];
        if (site_lp != nullptr) site_lp[(int64_t)v * K + k] = acc;
        t += acc;
      } else {
        slot_grad[(int64_t)(v - A.num_sites) * K + k] = (float)(acc * A.slot_scale);
      }
    }
  }
  if (gl == 0 && k < K && v_begin == 0 && A.ksum == 0) total[k] = (float)t;
}

// -------------------------------------------------------------------------------------------------
// Fused guide draws: sum the per-K-block dloc / dscale partials (fixed order, fp64).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_draw_reduce(const float* __restrict__ part, int64_t slices,
                                                     int64_t N, float* __restrict__ dloc,
                                                     float* __restrict__ dscale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double a = 0.0, b = 0.0;
  for (int64_t y = 0; y < slices; ++y) {
    a += (double)part[y * N + i];
    b += (double)part[(slices + y) * N + i];
  }
  dloc[i] = (float)a;
  dscale[i] = (float)b;
}

// -------------------------------------------------------------------------------------------------
// Backward rescale of speculative dense gradients.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scale_rows(float* __restrict__ x, int64_t sk, int64_t si,
                                                    int64_t K, int64_t N,
                                                    const float* __restrict__ g, float g0,
                                                    int64_t rows_per_block) {
  const int64_t k0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t k1 = min(K, k0 + rows_per_block);
  bool all_same = true;
  for (int64_t k = k0; k < k1; ++k) all_same &= (g[k] == g0);
  if (all_same) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int64_t k = k0; k < k1; ++k) {
    const float f = g[k] / g0;
    if (f != 1.0f) x[k * sk + i * si] *= f;
  }
}

}  // namespace mi

size_t mi_finalize_scratch_bytes(int64_t nseg, int64_t K, int nv) {
  if (nseg <= 2 * mi::kFinChunk) return 0;
  return (size_t)nv * (size_t)ceil_div(nseg, mi::kFinChunk) * (size_t)K * sizeof(double);
}

int mi_launch_finalize(const float* part, int64_t nseg, int64_t K, int num_sites, int num_slots,
                       const double* scale, double slot_scale, float* total, double* site_lp,
                       float* slot_grad, double* scratch, hipStream_t stream, int rank1,
                       int ksum) {
  if (num_sites > MI_MAX_SITES) return MI_EINVAL;
  mi::FinalizeArgs A{};
  A.num_sites = num_sites;
  A.num_slots = num_slots;
  A.rank1 = rank1;
  A.ksum = ksum;
  A.slot_scale = slot_scale;
  for (int i = 0; i < num_sites; ++i) A.scale[i] = scale[i];
  const int nv = num_sites + num_slots;
  const unsigned gx = (unsigned)ceil_div(K, mi::kFinK);
  const unsigned gy = num_sites == 1 ? (unsigned)nv : 1u;
  if (scratch != nullptr && mi_finalize_scratch_bytes(nseg, K, nv) != 0 && rank1 == 0 && ksum == 0) {
    // long segment lists: chunks of segments in parallel, then the chunk sums
    const int64_t nchunk = ceil_div(nseg, mi::kFinChunk);
    hipLaunchKernelGGL(mi::k_finalize_chunks, dim3(gx, (unsigned)nv, (unsigned)nchunk),
                       dim3(mi::kFinK * mi::kFinG), 0, stream, part, nseg, K, scratch);
    hipLaunchKernelGGL(mi::k_finalize<double>, dim3(gx, gy), dim3(mi::kFinK * mi::kFinG), 0,
                       stream, scratch, nchunk, K, A, total, site_lp, slot_grad);
  } else {
    hipLaunchKernelGGL(mi::k_finalize<float>, dim3(gx, gy), dim3(mi::kFinK * mi::kFinG), 0,
                       stream, part, nseg, K, A, total, site_lp, slot_grad);
  }
  return to_code(hipGetLastError());
}

int mi_reduce_launch_slots(const mi_reduce* r, void* stream) {
  if (r == nullptr || r->part == nullptr || r->nseg < 1 || r->K < 1 || r->ksum == 0 ||
      r->num_sites < 1 || r->num_sites > MI_MAX_SITES || r->num_slots < 0 ||
      (r->num_slots > 0 && r->slot_grad == nullptr) || r->nseg > MI_REDUCE_MAX_SEG)
    return MI_EINVAL;
  if (r->num_slots == 0) return 0;
  return mi_launch_finalize(r->part, r->nseg, r->K, r->num_sites, r->num_slots, r->scale,
                            r->slot_scale, r->total, nullptr, r->slot_grad, nullptr,
                            static_cast<hipStream_t>(stream), r->rank1, r->ksum);
}

int mi_launch_draw_reduce(const float* part, int64_t slices, int64_t N, float* dloc, float* dscale,
                          hipStream_t stream) {
  hipLaunchKernelGGL(mi::k_draw_reduce, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, stream,
                     part, slices, N, dloc, dscale);
  return to_code(hipGetLastError());
}

extern "C" {

int mi_reduce_launch(const mi_reduce* r, void* stream) {
  if (r == nullptr || r->part == nullptr || r->nseg < 1 || r->K < 1 || r->total == nullptr ||
      r->num_sites < 1 || r->num_sites > MI_MAX_SITES || r->num_slots < 0 ||
      (r->num_slots > 0 && r->slot_grad == nullptr) || r->nseg > MI_REDUCE_MAX_SEG)
    return MI_EINVAL;
  // particle-summed values have no [nseg, K] block to finalize (mi_reduce.ksum)
  if (r->ksum != 0) return MI_EUNSUPPORTED;
  // nseg <= MI_REDUCE_MAX_SEG: the one-launch finalize (no chunk scratch)
  return mi_launch_finalize(r->part, r->nseg, r->K, r->num_sites, r->num_slots, r->scale,
                            r->slot_scale, r->total, r->site_lp, r->slot_grad, nullptr,
                            static_cast<hipStream_t>(stream), r->rank1);
}

int mi_scale_rows(float* x, int64_t stride_k, int64_t stride_i, int64_t K, int64_t N,
                  const float* g, float g0, void* stream) {
  if (x == nullptr || g == nullptr || K < 1 || N < 1 || g0 == 0.0f) return MI_EINVAL;
  const int64_t rows = 64;
  dim3 grid((unsigned)ceil_div(N, 256), (unsigned)ceil_div(K, rows));
  hipLaunchKernelGGL(mi::k_scale_rows, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     stride_k, stride_i, K, N, g, g0, rows);
  return to_code(hipGetLastError());
}

}  // extern "C"
