// The Categorical row site: log p of integer values under per-(particle, element) logit rows, and
// the dense gradient with respect to the logits. Restates torch/distributions/categorical.py
// (file:line cited at the kernel).
#include "common.hpp"

#include <cmath>

#include "internal.hpp"
namespace mi {

// -------------------------------------------------------------------------------------------------
// Categorical: normalisation (categorical.py:74-78, logits - logsumexp) and gather
// (categorical.py:150-156) of one (particle, element) row per lane, lanes along elements. The row's
// C logits are read twice (max, then the exponentials; the second pass hits L1/L2). Gradient with
// respect to the given logits, dense: g * (onehot(v) - softmax) -- exact for raw logits, and for
// already normalised ones (whose logsumexp is 0) the same vector autograd's normalisation backward
// passes through unchanged.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_categorical(
    const float* __restrict__ logits, int64_t sk, int64_t si, int64_t sc, int64_t K, int64_t N,
    int64_t C, const int64_t* __restrict__ value, int64_t vsk, int64_t vsi,
    const uint8_t* __restrict__ mask, int64_t msi, float gscale, float* __restrict__ dlogits,
    float* __restrict__ part, int64_t nseg, uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t k = blockIdx.y;
  uint32_t fl = 0u;
  if (seg < nseg) {
    float acc = 0.0f;
    for (int e = 0; e < 16; ++e) {
      const int64_t i = seg * 1024 + e * 64 + lane;
      if (i >= N) break;
      const bool obs = mask == nullptr || mask[i * msi] != 0;
      const int64_t v = value[k * vsk + i * vsi];
      const bool ok = v >= 0 && v < C;
      fl |= (obs && !ok) ? MI_FLAG_SUPPORT : 0u;
      const float* row = logits + k * sk + i * si;
      float* drow = dlogits == nullptr ? nullptr : dlogits + k * sk + i * si;
      if (!(obs && ok)) {   // masked lanes: value and gradient 0 (util.py:85-90)
        if (drow != nullptr)
          for (int64_t c = 0; c < C; ++c) drow[c * sc] = 0.0f;
        continue;
      }
      float mx = -INFINITY;
      for (int64_t c = 0; c < C; ++c) mx = fmaxf(mx, row[c * sc]);
      const float shift = isinf(mx) ? 0.0f : mx;   // torch.logsumexp's all--inf guard
      float se = 0.0f;
      for (int64_t c = 0; c < C; ++c) se += expf(row[c * sc] - shift);
      const float lse = logf(se) + shift;
      acc += row[v * sc] - lse;
      if (drow != nullptr) {
        const float inv = 1.0f / se;
        for (int64_t c = 0; c < C; ++c) {
          const float soft = expf(row[c * sc] - shift) * inv;
          drow[c * sc] = gscale * ((c == v ? 1.0f : 0.0f) - soft);
        }
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) part[seg * K + k] = acc;
  }
  publish_flags(flags, fl);
}

__global__ void k_categorical_finalize(const float* __restrict__ part, int64_t nseg, int64_t K,
                                       double scale, float* __restrict__ total) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double acc = 0.0;
  for (int64_t g = 0; g < nseg; ++g) acc += (double)part[g * K + k];
  total[k] = (float)(acc * scale);
}

}  // namespace mi

extern "C" {

int mi_categorical_workspace_bytes(int64_t K, int64_t N, size_t* bytes) {
  if (K < 1 || N < 1 || bytes == nullptr) return MI_EINVAL;
  *bytes = (size_t)ceil_div(N, 1024) * (size_t)K * sizeof(float);
  return 0;
}

int mi_categorical_forward(const float* logits, int64_t stride_k, int64_t stride_i,
                           int64_t stride_c, int64_t K, int64_t N, int64_t C,
                           const int64_t* value, int64_t value_stride_k, int64_t value_stride_i,
                           const uint8_t* mask, int64_t mask_stride_i, double scale, float g0,
                           float* dlogits, void* workspace, size_t workspace_bytes, float* total,
                           uint32_t* flags, void* stream) {
  if (logits == nullptr || value == nullptr || total == nullptr || flags == nullptr || K < 1 ||
      N < 1 || C < 1)
    return MI_EINVAL;
  size_t need = 0;
  mi_categorical_workspace_bytes(K, N, &need);
  if (workspace == nullptr || workspace_bytes < need) return MI_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return to_code(e);
  const int64_t nseg = ceil_div(N, 1024);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(mi::k_categorical, dim3((unsigned)ceil_div(nseg, 4), (unsigned)K), dim3(256),
                     0, s, logits, stride_k, stride_i, stride_c, K, N, C, value, value_stride_k,
                     value_stride_i, mask, mask_stride_i, (float)(g0 * scale), dlogits, part, nseg,
                     flags);
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_categorical_finalize, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, s,
                     part, nseg, K, scale, total);
  return to_code(hipGetLastError());
}

}  // extern "C"
