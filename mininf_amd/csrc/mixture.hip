// Normal-mixture site: the density of MixtureSameFamily(Categorical(logits), Normal(loc, scale))
// with the assignment summed out, and its four gradients.
//
// Replaces, for float32 parameters and C = the number of components <= MI_MIXTURE_MAX_C,
// MixtureSameFamily.log_prob (torch/distributions/mixture_same_family.py:169-179: _pad, the
// component log_prob at [.., C], log_softmax of the mixture logits, their sum and a logsumexp) and
// its autograd.
//
// Layout: the row groups of row_groups.hpp, one (particle, row) per group, lanes striding over the
// components. No atomics (the validation word's OR aside, whose result does not depend on order):
// every sum has a fixed order, so results do not depend on the launch.
#include "internal.hpp"
#include "row_groups.hpp"

namespace mi {

// A [K, N, C] parameter read where it lies: any of the strides may be 0.
struct MixParam {
  const float* p;
  int64_t sk, si, sc;
};

// u_c = logits_c - log scale_c - 1/2 log 2 pi - 1/2 z_c^2: t_c before the logits are normalised
// (t_c = u_c - logsumexp logits).
MI_DEV float mix_term(float l, float mu, float s, float x, float* z_out) {
  const float z = (x - mu) / s;
  *z_out = z;
  return l - logf(s) - kHalfLog2Pi - 0.5f * z * z;
}

// -------------------------------------------------------------------------------------------------
// Per (k, i), with m = log_softmax(logits) and z_c = (x - loc_c) / scale_c:
//   t_c = m_c - log scale_c - 1/2 log 2 pi - 1/2 z_c^2,  l = logsumexp_c t_c,  r_c = exp(t_c - l)
// evaluated as l = (max u + log sum exp(u - max u)) - (max logits + log sum exp(logits - max)):
// the first pass reads both maxima, the second adds both sums (fp32, lanes then the shuffle tree),
// the third writes the gradients. The two logarithms and the row's accumulation are fp64.
// Speculative gradients (gscale = g0 * scale folded in, zeros on masked rows):
//   d/dlogits_c = r_c - exp(m_c)        d/dloc_c = r_c z_c / scale_c
//   d/dscale_c  = r_c (z_c^2 - 1) / scale_c        d/dx = -sum_c r_c z_c / scale_c
// A component of logit -inf has u_c = -inf: r_c = exp(m_c) = 0 and its gradients are zeros.
// Validation: MI_FLAG_PARAM unless every scale_c > 0, no logit is NaN and one is finite;
// MI_FLAG_SUPPORT for a NaN value (the Normal site's check). Masked rows raise nothing.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void k_mixture_normal(
    const MixParam L, const MixParam M, const MixParam S, int64_t K, int64_t N, int64_t C,
    const float* __restrict__ value, int64_t vsk, int64_t vsi, const uint8_t* __restrict__ mask,
    int64_t msi, float gscale, float* __restrict__ dlogits, float* __restrict__ dloc,
    float* __restrict__ dscale, float* __restrict__ dvalue, double* __restrict__ row_lp,
    uint32_t* __restrict__ flags, int W, int shift) {
  const RowLane rl = row_lane(shift);
  const bool valid = rl.row < K * N;
  const int64_t k = valid ? rl.row / N : 0, i = valid ? rl.row - k * N : 0;
  const bool obs = valid && (mask == nullptr || mask[i * msi] != 0);
  const float* lg = L.p + k * L.sk + i * L.si;
  const float* mu = M.p + k * M.sk + i * M.si;
  const float* sd = S.p + k * S.sk + i * S.si;
  const float x = obs ? value[k * vsk + i * vsi] : 0.0f;
  const float ninf = -__builtin_inff();
  float lmax = ninf, umax = ninf;
  uint32_t fl = 0u;
  int finite = 0;
  if (obs) {
    fl |= (x != x) ? MI_FLAG_SUPPORT : 0u;
    for (int64_t c = rl.sub; c < C; c += W) {
      const float l = lg[c * L.sc], s = sd[c * S.sc];
      float z;
      const float u = mix_term(l, mu[c * M.sc], s, x, &z);
      fl |= (!(s > 0.0f) || l != l) ? MI_FLAG_PARAM : 0u;
      finite |= fabsf(l) < __builtin_inff() ? 1 : 0;
      lmax = fmaxf(lmax, l);
      umax = fmaxf(umax, u);
    }
  }
  lmax = group_max(lmax, W);
  umax = group_max(umax, W);
  finite = group_sum(finite, W);
  float sl = 0.0f, su = 0.0f;
  if (obs) {
    fl |= finite == 0 ? MI_FLAG_PARAM : 0u;
    for (int64_t c = rl.sub; c < C; c += W) {
      const float l = lg[c * L.sc];
      float z;
      const float u = mix_term(l, mu[c * M.sc], sd[c * S.sc], x, &z);
      sl += expf(l - lmax);
      su += expf(u - umax);
    }
  }
  sl = group_sum(sl, W);
  su = group_sum(su, W);
  if (valid && rl.sub == 0)
    row_lp[rl.row] = obs ? ((double)umax + log((double)su)) - ((double)lmax + log((double)sl)) : 0.0;
  const bool grads = dlogits != nullptr || dloc != nullptr || dscale != nullptr;
  float dx = 0.0f;
  if (valid && (grads || dvalue != nullptr)) {
    const float rsl = 1.0f / sl, rsu = 1.0f / su;
    for (int64_t c = rl.sub; c < C; c += W) {
      const int64_t o = rl.row * C + c;
      float dl = 0.0f, dm = 0.0f, ds = 0.0f;
      if (obs) {   // masked rows: value and gradients 0
        const float l = lg[c * L.sc], s = sd[c * S.sc];
        float z;
        const float u = mix_term(l, mu[c * M.sc], s, x, &z);
        const float r = expf(u - umax) * rsu;
        const float rz = r * z / s;
        dl = gscale * (r - expf(l - lmax) * rsl);
        dm = gscale * rz;
        ds = gscale * (r * (z * z - 1.0f) / s);
        dx += rz;
      }
      if (dlogits != nullptr) dlogits[o] = dl;
      if (dloc != nullptr) dloc[o] = dm;
      if (dscale != nullptr) dscale[o] = ds;
    }
  }
  dx = group_sum(dx, W);
  if (valid && rl.sub == 0 && dvalue != nullptr) dvalue[rl.row] = -gscale * dx;
  publish_flags(flags, fl);
}

}  // namespace mi

extern "C" {

int mi_mixture_normal_workspace_bytes(int64_t K, int64_t N, int64_t C, size_t* bytes) {
  if (!row_shape_ok(K, N, C) || bytes == nullptr) return MI_EINVAL;
  if (C > MI_MIXTURE_MAX_C) return MI_EUNSUPPORTED;
  *bytes = (size_t)K * (size_t)N * sizeof(double);
  return 0;
}

int mi_mixture_normal_forward(const float* logits, int64_t logits_stride_k,
                              int64_t logits_stride_i, int64_t logits_stride_c, const float* loc,
                              int64_t loc_stride_k, int64_t loc_stride_i, int64_t loc_stride_c,
                              const float* component_scale, int64_t scale_stride_k,
                              int64_t scale_stride_i, int64_t scale_stride_c, int64_t K, int64_t N,
                              int64_t C, const float* value, int64_t value_stride_k,
                              int64_t value_stride_i, const uint8_t* mask, int64_t mask_stride_i,
                              double scale, float g0, float* dlogits, float* dloc, float* dscale,
                              float* dvalue, void* workspace, size_t workspace_bytes, float* total,
                              uint32_t* flags, void* stream) {
  if (logits == nullptr || loc == nullptr || component_scale == nullptr || value == nullptr ||
      total == nullptr || flags == nullptr || !row_shape_ok(K, N, C))
    return MI_EINVAL;
  if (C > MI_MIXTURE_MAX_C) return MI_EUNSUPPORTED;
  size_t need = 0;
  mi_mixture_normal_workspace_bytes(K, N, C, &need);
  if (workspace == nullptr || workspace_bytes < need) return MI_EWORKSPACE;
  int W, shift;
  row_group(C, &W, &shift);
  const int64_t blocks = row_blocks(K * N, W);
  if (blocks == 0) return MI_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return to_code(e);
  double* row_lp = static_cast<double*>(workspace);
  const mi::MixParam L{logits, logits_stride_k, logits_stride_i, logits_stride_c};
  const mi::MixParam M{loc, loc_stride_k, loc_stride_i, loc_stride_c};
  const mi::MixParam S{component_scale, scale_stride_k, scale_stride_i, scale_stride_c};
  hipLaunchKernelGGL(mi::k_mixture_normal, dim3((unsigned)blocks), dim3(mi::kRowThreads), 0, s, L,
                     M, S, K, N, C, value, value_stride_k, value_stride_i, mask, mask_stride_i,
                     (float)(g0 * scale), dlogits, dloc, dscale, dvalue, row_lp, flags, W, shift);
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_rows_finalize, dim3((unsigned)ceil_div(K, mi::kRowThreads / 64)),
                     dim3(mi::kRowThreads), 0, s, row_lp, K, N, scale, total);
  return to_code(hipGetLastError());
}

}  // extern "C"
