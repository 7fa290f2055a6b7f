// Dirichlet: site density, guide sampling with its backward, and entropy.
//
// Replaces, for a float32 Dirichlet of C = event_shape[0] <= MI_DIRICHLET_MAX_C categories,
//   * Dirichlet.log_prob (torch/distributions/dirichlet.py:90-97) and its autograd,
//   * Dirichlet.rsample (dirichlet.py:85-88 -> _Dirichlet, :23-36: torch._sample_dirichlet and
//     _Dirichlet_backward, :17-20, i.e. torch._dirichlet_grad, ATen/native/Distributions.h
//     dirichlet_grad_one -- the per-component function beta_grad.hpp restates),
//   * Dirichlet.entropy (dirichlet.py:122-130) and its autograd.
//
// Layout of every kernel that walks rows: the row groups of row_groups.hpp. No atomics (the
// validation word's OR aside, whose result does not depend on order): every sum has a fixed order,
// so results do not depend on the launch.
#include "beta_grad.hpp"
#include "gamma_sample.hpp"
#include "internal.hpp"
#include "row_groups.hpp"

#include <algorithm>

namespace mi {

constexpr int kDirThreads = kRowThreads;

// fp64 trigamma: recurrence up to x >= 10, then the asymptotic (Bernoulli-number) series. NaN
// unless x > 0 (concentrations are positive; a bad one must not spin the recurrence).
MI_DEV double trigamma(double x) {
  if (!(x > 0.0)) return __builtin_nan("");
  double acc = 0.0;
  while (x < 10.0) {
    acc += 1.0 / (x * x);
    x += 1.0;
  }
  const double r = 1.0 / (x * x);
  return acc + 1.0 / x + 0.5 * r +
         r / x * (1.0 / 6 - r * (1.0 / 30 - r * (1.0 / 42 - r * (1.0 / 30 - r * (5.0 / 66)))));
}

// -------------------------------------------------------------------------------------------------
// Site density. Per (k, i), dirichlet.py:93-97:
//   sum_c xlogy(a_c - 1, x_c) + lgamma(sum_c a_c) - sum_c lgamma(a_c)
// with the row sum a0 in fp32 (as torch's concentration.sum(-1)), the lgamma terms and the row's
// accumulation in fp64. Speculative gradients (gscale = g0 * scale folded in, zeros on masked rows):
//   d/da_c = log x_c + psi(a0) - psi(a_c)   (digamma in fp64)
//   d/dx_c = (a_c - 1) / x_c
// following torch's autograd formulas of xlogy (tools/autograd/derivatives.yaml, xlogy.Tensor:
// self: at::xlogy(grad, other).masked_fill((self == 0.) & (other <= 0.), 0.), other: grad * self /
// other): at a_c = 1 the log x_c term is dropped where x_c <= 0, and d/dx_c is 0 / x_c.
// Validation: MI_FLAG_PARAM unless every a_c > 0 (independent(positive, 1)); MI_FLAG_SUPPORT unless
// every x_c >= 0 and |sum_c x_c - 1| < 1e-6 (constraints.py, _Simplex.check) -- the sum in fp64, so
// that the check never rejects a row for the order this kernel adds it in.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDirThreads) void k_dirichlet(
    const float* __restrict__ conc, int64_t sk, int64_t si, int64_t sc, int64_t K, int64_t N,
    int64_t C, const float* __restrict__ value, int64_t vsk, int64_t vsi, int64_t vsc,
    const uint8_t* __restrict__ mask, int64_t msi, float gscale, float* __restrict__ dconc,
    float* __restrict__ dvalue, double* __restrict__ row_lp, uint32_t* __restrict__ flags, int W,
    int shift) {
  const RowLane rl = row_lane(shift);
  const bool valid = rl.row < K * N;
  const int64_t k = valid ? rl.row / N : 0, i = valid ? rl.row - k * N : 0;
  const bool obs = valid && (mask == nullptr || mask[i * msi] != 0);
  const float* a = conc + k * sk + i * si;
  const float* x = value + k * vsk + i * vsi;
  float a0 = 0.0f;
  double sx = 0.0, lp = 0.0;
  uint32_t fl = 0u;
  if (obs) {
    for (int64_t c = rl.sub; c < C; c += W) {
      const float av = a[c * sc], xv = x[c * vsc];
      a0 += av;
      sx += (double)xv;
      fl |= !(av > 0.0f) ? MI_FLAG_PARAM : 0u;
      fl |= !(xv >= 0.0f) ? MI_FLAG_SUPPORT : 0u;
      lp += (double)xlogy(av - 1.0f, xv) - lgamma((double)av);
    }
  }
  a0 = group_sum(a0, W);
  sx = group_sum(sx, W);
  lp = group_sum(lp, W);
  if (obs) {
    fl |= !(fabs(sx - 1.0) < 1e-6) ? MI_FLAG_SUPPORT : 0u;
    lp += lgamma((double)a0);
  }
  if (valid && rl.sub == 0) row_lp[rl.row] = obs ? lp : 0.0;
  if (valid && (dconc != nullptr || dvalue != nullptr)) {
    const double psi0 = obs ? digamma((double)a0) : 0.0;
    for (int64_t c = rl.sub; c < C; c += W) {
      const int64_t o = rl.row * C + c;
      float da = 0.0f, dx = 0.0f;
      if (obs) {   // masked rows: value and gradients 0 (util.py:85-90)
        const float av = a[c * sc], xv = x[c * vsc];
        const float am1 = av - 1.0f;
        const float lx = (am1 == 0.0f && xv <= 0.0f) ? 0.0f : logf(xv);
        da = gscale * (lx + (float)(psi0 - digamma((double)av)));
        dx = gscale * (am1 / xv);
      }
      if (dconc != nullptr) dconc[o] = da;
      if (dvalue != nullptr) dvalue[o] = dx;
    }
  }
  publish_flags(flags, fl);
}

// -------------------------------------------------------------------------------------------------
// Guide draws: x[k, n, c] = g_c / sum_j g_j with g_c the standard Gamma(a[n, c]) variate of the
// Gamma sampler's sub-stream (2) at element n C + c -- the variates mi_gamma_rsample draws for the
// flattened concentrations -- or g_in[k, n, c] (parity mode). The row sum is taken in fp64 and each
// component divided once, then clamped to [FLT_MIN, 1 - 2^-24] as torch's _sample_dirichlet
// clamps (ATen/native/Distributions.cpp, _s_dirichlet_cpu: min_value / max_value). A row whose
// variates all underflow becomes the (clamped) one-hot of its largest concentration, the choice
// k_beta_rsample makes. The variates pass through x itself (each lane re-reads what it wrote).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDirThreads) void k_dirichlet_rsample(
    const float* __restrict__ conc, int64_t K, int64_t N, int64_t C, uint64_t seed, uint64_t step,
    const uint64_t* __restrict__ step_dev, uint32_t stream_id, int64_t poff,
    const float* __restrict__ g_in, float* x, int W, int shift) {
  const RowLane rl = row_lane(shift);
  const bool valid = rl.row < K * N;
  const int64_t k = valid ? rl.row / N : 0, n = valid ? rl.row - k * N : 0;
  const float* a = conc + n * C;
  float* out = x + rl.row * C;
  if (step_dev != nullptr) step += *step_dev;
  double s = 0.0;
  float amax = -INFINITY;
  int cmax = (int)C;
  if (valid) {
    for (int64_t c = rl.sub; c < C; c += W) {
      const float av = a[c];
      float g;
      if (g_in != nullptr) {
        g = g_in[rl.row * C + c];
      } else {
        Stream rng{seed, step, stream_id, 2u, (uint64_t)(n * C + c), (uint64_t)(poff + k)};
        g = sample_gamma(av, rng);
      }
      out[c] = g;
      s += (double)g;
      if (av > amax) {
        amax = av;
        cmax = (int)c;
      }
    }
  }
  s = group_sum(s, W);
  // the first largest concentration of the row
  for (int offset = W >> 1; offset > 0; offset >>= 1) {
    const float oa = __shfl_xor(amax, offset, kWave);
    const int oc = __shfl_xor(cmax, offset, kWave);
    if (oa > amax || (oa == amax && oc < cmax)) {
      amax = oa;
      cmax = oc;
    }
  }
  if (!valid) return;
  const float lo = 1.17549435e-38f, hi = 0.99999994f;
  for (int64_t c = rl.sub; c < C; c += W) {
    const float v = s > 0.0 ? (float)((double)out[c] / s) : (c == cmax ? 1.0f : 0.0f);
    out[c] = fminf(hi, fmaxf(lo, v));
  }
}

// Backward, first launch: dot[k, n] = sum_j x[k, n, j] dx[k, n, j] (fp64), and from the k = 0 rows
// the parameter-only terms tot[n] = sum_c a[n, c] (fp32, concentration.sum(-1), dirichlet.py:18)
// and psi_tot[n] = digamma(tot[n]).
__global__ __launch_bounds__(kDirThreads) void k_dirichlet_bwd_dot(
    const float* __restrict__ dx, int64_t dsk, int64_t dsi, int64_t dsc,
    const float* __restrict__ x, const float* __restrict__ conc, int64_t K, int64_t N, int64_t C,
    double* __restrict__ dot, float* __restrict__ tot, double* __restrict__ psi_tot, int W,
    int shift) {
  const RowLane rl = row_lane(shift);
  const bool valid = rl.row < K * N;
  const int64_t k = valid ? rl.row / N : 0, n = valid ? rl.row - k * N : 0;
  double s = 0.0;
  float a0 = 0.0f;
  if (valid) {
    for (int64_t c = rl.sub; c < C; c += W) {
      s += (double)x[rl.row * C + c] * (double)dx[k * dsk + n * dsi + c * dsc];
      if (k == 0) a0 += conc[n * C + c];
    }
  }
  s = group_sum(s, W);
  a0 = group_sum(a0, W);
  if (valid && rl.sub == 0) {
    dot[rl.row] = s;
    if (k == 0) {
      tot[n] = a0;
      psi_tot[n] = digamma((double)a0);
    }
  }
}

// Backward, second launch (_Dirichlet_backward, dirichlet.py:17-20), reduced over the particle
// rows [k0, k1) of this block's slice per element e = n C + c:
//   part[slice, e] = sum_k dirichlet_grad(x_kc, a_c, tot) (dx_kc - dot_k)
// Blocked like k_beta_rsample_bwd: TI element lanes x 256 / TI particle lanes, combined in a fixed
// order through LDS. digamma(a_c) once per element and block, digamma(tot) from the first launch.
__global__ __launch_bounds__(kDirThreads) void k_dirichlet_rsample_bwd(
    const float* __restrict__ dx, int64_t dsk, int64_t dsi, int64_t dsc,
    const float* __restrict__ x, const float* __restrict__ conc, const double* __restrict__ dot,
    const float* __restrict__ tot, const double* __restrict__ psi_tot, int64_t K, int64_t N,
    int64_t C, float* __restrict__ part, int64_t rows_per_block, int ti) {
  __shared__ double red[kDirThreads];
  const int tx = threadIdx.x % ti, ty = threadIdx.x / ti, tk = kDirThreads / ti;
  const int64_t e = (int64_t)blockIdx.x * ti + tx;
  const int64_t k0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t k1 = min(K, k0 + rows_per_block);
  double acc = 0.0;
  if (e < N * C) {
    const int64_t n = e / C, c = e - n * C;
    const float a = conc[e], t = tot[n];
    const double psi_a = digamma((double)a), psi_t = psi_tot[n];
    for (int64_t k = k0 + ty; k < k1; k += tk) {
      const double d = (double)dx[k * dsk + n * dsi + c * dsc] - dot[k * N + n];
      if (d == 0.0) continue;
      acc += dirichlet_grad((double)x[(k * N + n) * C + c], (double)a, (double)t, psi_a, psi_t) * d;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (ty == 0 && e < N * C) {
    double sum = 0.0;
    for (int r = 0; r < tk; ++r) sum += red[r * ti + tx];
    part[blockIdx.y * N * C + e] = (float)sum;
  }
}

// out[e] = sum over the slices of part[slice, e] (fixed order, fp64).
__global__ __launch_bounds__(kDirThreads) void k_dirichlet_sum_slices(
    const float* __restrict__ part, int64_t slices, int64_t M, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kDirThreads + threadIdx.x;
  if (e >= M) return;
  double acc = 0.0;
  for (int64_t s = 0; s < slices; ++s) acc += (double)part[s * M + e];
  out[e] = (float)acc;
}

// -------------------------------------------------------------------------------------------------
// Entropy (dirichlet.py:122-130) summed over the rows, and its gradient, fp64 throughout:
//   H       = sum_n [sum_c lgamma(a_c) - lgamma(a0) - (C - a0) psi(a0) - sum_c (a_c - 1) psi(a_c)]
//   dH/da_c = (a0 - C) psi'(a0) - (a_c - 1) psi'(a_c)
// One block: its 256 / W row groups stride over the rows, each keeping its own fp64 sum; the
// groups' sums meet in LDS in group order.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDirThreads) void k_dirichlet_entropy(
    const float* __restrict__ conc, int64_t N, int64_t C, float* __restrict__ entropy,
    float* __restrict__ dconc, int W, int shift) {
  __shared__ double red[kDirThreads];
  const int sub = threadIdx.x & (W - 1), group = threadIdx.x >> shift, groups = kDirThreads >> shift;
  double acc = 0.0;
  for (int64_t n0 = 0; n0 < N; n0 += groups) {   // (uniform trip count: the shuffles need every lane)
    const int64_t n = n0 + group;
    const bool valid = n < N;
    const float* a = conc + n * C;
    double a0 = 0.0, h = 0.0;
    if (valid) {
      for (int64_t c = sub; c < C; c += W) {
        const double av = (double)a[c];
        a0 += av;
        h += lgamma(av) - (av - 1.0) * digamma(av);
      }
    }
    a0 = group_sum(a0, W);
    h = group_sum(h, W);
    if (!valid) continue;
    if (sub == 0) acc += h - lgamma(a0) - ((double)C - a0) * digamma(a0);
    if (dconc != nullptr) {
      const double t0 = (a0 - (double)C) * trigamma(a0);
      for (int64_t c = sub; c < C; c += W) {
        const double av = (double)a[c];
        dconc[n * C + c] = (float)(t0 - (av - 1.0) * trigamma(av));
      }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) sum += red[g << shift];
    entropy[0] = (float)sum;
  }
}

}  // namespace mi

namespace {

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int mi_dirichlet_workspace_bytes(int64_t K, int64_t N, int64_t C, size_t* bytes) {
  if (!row_shape_ok(K, N, C) || bytes == nullptr) return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  *bytes = (size_t)K * (size_t)N * sizeof(double);
  return 0;
}

int mi_dirichlet_forward(const float* concentration, int64_t stride_k, int64_t stride_i,
                         int64_t stride_c, int64_t K, int64_t N, int64_t C, const float* value,
                         int64_t value_stride_k, int64_t value_stride_i, int64_t value_stride_c,
                         const uint8_t* mask, int64_t mask_stride_i, double scale, float g0,
                         float* dconcentration, float* dvalue, void* workspace,
                         size_t workspace_bytes, float* total, uint32_t* flags, void* stream) {
  if (concentration == nullptr || value == nullptr || total == nullptr || flags == nullptr ||
      !row_shape_ok(K, N, C))
    return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  size_t need = 0;
  mi_dirichlet_workspace_bytes(K, N, C, &need);
  if (workspace == nullptr || workspace_bytes < need) return MI_EWORKSPACE;
  int W, shift;
  row_group(C, &W, &shift);
  const int64_t blocks = row_blocks(K * N, W);
  if (blocks == 0) return MI_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return to_code(e);
  double* row_lp = static_cast<double*>(workspace);
  hipLaunchKernelGGL(mi::k_dirichlet, dim3((unsigned)blocks), dim3(mi::kDirThreads), 0, s,
                     concentration, stride_k, stride_i, stride_c, K, N, C, value, value_stride_k,
                     value_stride_i, value_stride_c, mask, mask_stride_i, (float)(g0 * scale),
                     dconcentration, dvalue, row_lp, flags, W, shift);
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_rows_finalize,
                     dim3((unsigned)ceil_div(K, mi::kDirThreads / 64)), dim3(mi::kDirThreads), 0,
                     s, row_lp, K, N, scale, total);
  return to_code(hipGetLastError());
}

int mi_dirichlet_rsample(const float* concentration, int64_t K, int64_t N, int64_t C,
                         uint64_t seed, uint64_t step, const uint64_t* step_device,
                         uint32_t stream_id, int64_t particle_offset, const float* g_in, float* x,
                         void* stream) {
  if (concentration == nullptr || x == nullptr || !row_shape_ok(K, N, C) || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  int W, shift;
  row_group(C, &W, &shift);
  const int64_t blocks = row_blocks(K * N, W);
  if (blocks == 0) return MI_EUNSUPPORTED;
  hipLaunchKernelGGL(mi::k_dirichlet_rsample, dim3((unsigned)blocks), dim3(mi::kDirThreads), 0,
                     static_cast<hipStream_t>(stream), concentration, K, N, C, seed, step,
                     step_device, stream_id, particle_offset, g_in, x, W, shift);
  return to_code(hipGetLastError());
}

int mi_dirichlet_rsample_backward_workspace_bytes(int64_t K, int64_t N, int64_t C,
                                                  size_t* bytes) {
  if (!row_shape_ok(K, N, C) || bytes == nullptr) return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  const BwdGeometry geo = bwd_geometry(K, N * C, mi::kDirThreads);
  // dot [K, N] and psi_tot [N] (fp64), tot [N] (fp32), then the slices' partial sums
  *bytes = (size_t)K * N * sizeof(double) + (size_t)N * sizeof(double) +
           align8((size_t)N * sizeof(float)) +
           (geo.slices > 1 ? (size_t)geo.slices * (size_t)(N * C) * sizeof(float) : 0);
  return 0;
}

int mi_dirichlet_rsample_backward(const float* dx, int64_t dx_stride_k, int64_t dx_stride_i,
                                  int64_t dx_stride_c, const float* x, const float* concentration,
                                  int64_t K, int64_t N, int64_t C, void* workspace,
                                  size_t workspace_bytes, float* dconcentration, void* stream) {
  if (dx == nullptr || x == nullptr || concentration == nullptr || dconcentration == nullptr ||
      !row_shape_ok(K, N, C))
    return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  size_t need = 0;
  mi_dirichlet_rsample_backward_workspace_bytes(K, N, C, &need);
  if (!workspace_ok(workspace, workspace_bytes, need)) return MI_EWORKSPACE;
  int W, shift;
  row_group(C, &W, &shift);
  const int64_t blocks = row_blocks(K * N, W);
  const BwdGeometry geo = bwd_geometry(K, N * C, mi::kDirThreads);
  if (blocks == 0 || geo.gx > kMaxGrid) return MI_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  double* dot = reinterpret_cast<double*>(base);
  double* psi_tot = dot + K * N;
  float* tot = reinterpret_cast<float*>(psi_tot + N);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(tot) +
                                         align8((size_t)N * sizeof(float)));
  float* out = slice_out(dconcentration, part, geo.slices, 0);
  hipLaunchKernelGGL(mi::k_dirichlet_bwd_dot, dim3((unsigned)blocks), dim3(mi::kDirThreads), 0, s,
                     dx, dx_stride_k, dx_stride_i, dx_stride_c, x, concentration, K, N, C, dot,
                     tot, psi_tot, W, shift);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_dirichlet_rsample_bwd, dim3((unsigned)geo.gx, (unsigned)geo.slices),
                     dim3(mi::kDirThreads), 0, s, dx, dx_stride_k, dx_stride_i, dx_stride_c, x,
                     concentration, dot, tot, psi_tot, K, N, C, out, geo.rows, geo.ti);
  e = hipGetLastError();
  if (e != hipSuccess || geo.slices == 1) return to_code(e);
  hipLaunchKernelGGL(mi::k_dirichlet_sum_slices,
                     dim3((unsigned)ceil_div(N * C, mi::kDirThreads)), dim3(mi::kDirThreads), 0, s,
                     part, geo.slices, N * C, dconcentration);
  return to_code(hipGetLastError());
}

int mi_dirichlet_entropy(const float* concentration, int64_t N, int64_t C, float* entropy,
                         float* dconcentration, void* stream) {
  if (concentration == nullptr || entropy == nullptr || !row_shape_ok(1, N, C)) return MI_EINVAL;
  if (C > MI_DIRICHLET_MAX_C) return MI_EUNSUPPORTED;
  int W, shift;
  row_group(C, &W, &shift);
  hipLaunchKernelGGL(mi::k_dirichlet_entropy, dim3(1), dim3(mi::kDirThreads), 0,
                     static_cast<hipStream_t>(stream), concentration, N, C, entropy,
                     dconcentration, W, shift);
  return to_code(hipGetLastError());
}

}  // extern "C"
