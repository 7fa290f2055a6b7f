// The BCAST launch shape of a site group (sites.hip): one site whose parameters are per-particle
// scalars and whose value is shared data x[i]. Two kernels -- k_bcast_prep + k_site_bcast (Normal,
// Beta, masked or strided Bernoulli: the value chunk staged in LDS) and k_site_bcast_smem (Bernoulli
// over unmasked contiguous data, the C2 hot path: scalar loads, or the int8 matrix cores for 0/1
// chunks) -- and the host policy that chooses between them and shapes their launches. The planner
// reaches this unit through bcast_site.hpp; the partials both kernels write are reduced by
// k_finalize (reduce.hip) or by the ELBO forward.
#include "beta_grad.hpp"
#include "common.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "bcast_site.hpp"
#include "internal.hpp"
namespace mi {

// -------------------------------------------------------------------------------------------------
// BCAST: one site, parameters are per-particle scalars (or constants), the value is shared data.
// -------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

MI_DEV float role_scalar(const mi_group& G, const mi_site& st, int q, int64_t k) {
  const int o = st.operand[q];
  if (o < 0) return st.constant[q];
  const mi_operand& op = G.operands[o];
  return op.data[k * op.stride_k];
}

MI_DEV float block_sum(float v, float* scratch) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[wave] = v;
  __syncthreads();
  float out = 0.0f;
#pragma unroll
  for (int w = 0; w < kBcastThreads / 64; ++w) out += scratch[w];
  return out;
}

// The same in fp64: lanes of a wave (butterfly), then the waves in order.
MI_DEV double block_sum(double v, double* scratch) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[wave] = v;
  __syncthreads();
  double out = 0.0;
#pragma unroll
  for (int w = 0; w < kBcastThreads / 64; ++w) out += scratch[w];
  return out;
}

// N block sums in one barrier round: each by block_sum's tree (the same bits), `scratch` N times
// as long.
template <int N, typename T>
MI_DEV void block_sum_n(T (&v)[N], T* scratch) {
  constexpr int kWaves = kBcastThreads / 64;
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) scratch[j * kWaves + wave] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    T out = (T)0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) out += scratch[j * kWaves + w];
    v[j] = out;
  }
}

// Per-particle constants of a BCAST site, computed once per particle (not once per element chunk):
//   Bernoulli: l, dl/dparam, softplus(l), sigmoid(l)
//   Normal:    loc, scale, log(scale) + log sqrt(2 pi)
//   Beta:      a - 1, b - 1, lgamma(a + b) - lgamma(a) - lgamma(b), psi(a+b) - psi(a), psi(a+b) - psi(b)
// laid out as prep[j * K + k]; parameter-constraint violations are flagged here.

template <int FAMILY>
__global__ __launch_bounds__(256) void k_bcast_prep(const mi_group G, float* __restrict__ prep,
                                                    uint32_t* __restrict__ flags) {
  const mi_site& st = G.sites[0];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t fl = 0u;
  if (k < G.K) {
    const float a = role_scalar(G, st, 0, k), b = role_scalar(G, st, 1, k);
    float c[kPrep] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool bad;
    if (FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS) {
      float l = a, dl = 1.0f;
      if (FAMILY == MI_BERNOULLI_PROBS) {
        bad = !(a >= 0.0f && a <= 1.0f);
        bernoulli_probs_to_logits(a, l, dl);
      } else {
        bad = l != l;
      }
      // log p(x | l) = x l - softplus(l);  d/dl = x - sigmoid(l)   (bernoulli.py:121-125)
      const float t = expf(-fabsf(l));
      c[0] = l;
      c[1] = dl;
      c[2] = fmaxf(l, 0.0f) + log1pf(t);
      c[3] = l >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
    } else if (FAMILY == MI_NORMAL) {
      bad = !(b > 0.0f) || (a != a);
      c[0] = a;
      c[1] = b;
      c[2] = (float)((double)logf(b) + (double)kHalfLog2Pi);
    } else {
      bad = !(a > 0.0f) || !(b > 0.0f);
      const double psi_ab = digamma((double)a + (double)b);
      c[0] = a - 1.0f;
      c[1] = b - 1.0f;
      c[2] = (float)((double)lgammaf(a + b) - (double)lgammaf(a) - (double)lgammaf(b));
      c[3] = (float)(psi_ab - digamma((double)a));
      c[4] = (float)(psi_ab - digamma((double)b));
    }
    fl = bad ? MI_FLAG_PARAM : 0u;
#pragma unroll
    for (int j = 0; j < kPrep; ++j) prep[j * G.K + k] = c[j];
  }
  publish_flags(flags, fl);
}

// FAMILY in {MI_BERNOULLI_LOGITS, MI_BERNOULLI_PROBS, MI_NORMAL, MI_BETA}
template <int FAMILY, bool MASKED>
__global__ __launch_bounds__(kBcastThreads) void k_site_bcast(const mi_group G,
                                                              const float* __restrict__ prep,
                                                              float* __restrict__ part,
                                                              int64_t nchunk,
                                                              uint32_t* __restrict__ flags) {
  constexpr bool BERN = FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS;
  constexpr int NF = BERN ? 1 : 2;
  // Bernoulli stages each value twice, (x, x), so a 16-byte LDS read feeds packed FMAs directly.
  __shared__ float4 feat[NF][BERN ? kBcastChunk / 2 : kBcastChunk / 4];
  __shared__ float scratch[kBcastThreads / 64];
  __shared__ float sums[4];

  const mi_site& st = G.sites[0];
  const mi_operand& vop = G.operands[st.operand[2]];
  const int64_t c = blockIdx.x;
  const int64_t i0 = c * kBcastChunk;
  const int64_t len = min((int64_t)kBcastChunk, G.N - i0);

  // ---- stage: features of the value chunk, particle-independent sums, support flags ----------
  float* f0 = reinterpret_cast<float*>(feat[0]);
  float* f1 = reinterpret_cast<float*>(feat[NF - 1]);
  float s_m = 0.0f, s_a = 0.0f, s_b = 0.0f, s_zero = 0.0f, s_one = 0.0f;
  uint32_t fl = 0u;
  for (int j = threadIdx.x; j < kBcastChunk; j += kBcastThreads) {
    float v = 0.0f, m = 0.0f;
    if (j < len) {
      const int64_t i = i0 + j;
      v = vop.data[i * vop.stride_i];
      m = 1.0f;
      if (MASKED) m = st.mask[i * st.mask_stride_i] != 0 ? 1.0f : 0.0f;
    }
    const bool obs = m != 0.0f;
    if (FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS) {
      fl |= (obs && !(v == 0.0f || v == 1.0f)) ? MI_FLAG_SUPPORT : 0u;
      const float f = obs ? v : 0.0f;
      f0[2 * j] = f;
      f0[2 * j + 1] = f;
      s_a += f;
    } else if (FAMILY == MI_NORMAL) {
      fl |= (obs && v != v) ? MI_FLAG_SUPPORT : 0u;
      f0[j] = obs ? v : 0.0f;
      f1[j] = m;
    } else {  // MI_BETA: log v and log(1 - v); exact 0 / 1 values are counted separately
      fl |= (obs && !(v >= 0.0f && v <= 1.0f)) ? MI_FLAG_SUPPORT : 0u;
      const bool zero = obs && v == 0.0f, one = obs && v == 1.0f;
      const float la = (obs && !zero) ? logf(v) : 0.0f;
      const float lb = (obs && !one) ? logf(1.0f - v) : 0.0f;
      f0[j] = la;
      f1[j] = lb;
      s_a += la;
      s_b += lb;
      s_zero += zero ? 1.0f : 0.0f;
      s_one += one ? 1.0f : 0.0f;
    }
    s_m += m;
  }
  s_m = block_sum(s_m, scratch);
  s_a = block_sum(s_a, scratch);
  if (FAMILY == MI_BETA) {
    s_b = block_sum(s_b, scratch);
    s_zero = block_sum(s_zero, scratch);
    s_one = block_sum(s_one, scratch);
  }
  (void)sums;
  __syncthreads();

  // ---- per-particle element loop -------------------------------------------------------------
  const int64_t kbase = (int64_t)blockIdx.y * (kBcastThreads * kBcastP) + threadIdx.x;
  // Hoisted per-particle coefficients of the element loop (k_bcast_prep).
  const int64_t K = G.K;
  float ca[kBcastP], cb[kBcastP];
#pragma unroll
  for (int p = 0; p < kBcastP; ++p) {
    const int64_t k = min(kbase + p * kBcastThreads, K - 1);
    ca[p] = prep[k];
    cb[p] = prep[K + k];
  }

  double acc1[kBcastP], acc2[kBcastP];
#pragma unroll
  for (int p = 0; p < kBcastP; ++p) acc1[p] = acc2[p] = 0.0;

  // One quad of staged features against all P particles of this lane. `exact` quads hold four real
  // elements; the others (the chunk's tail) use the masked formulation, which is neutral for the
  // zero padding.
  auto quad = [&](const float4 x, const float4 y, float (&in1)[kBcastP], float (&in2)[kBcastP],
                  bool exact) {
    if (FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS) {
      // log p(x | l) = x l - softplus(l): one FMA per (particle, element)
#pragma unroll
      for (int p = 0; p < kBcastP; ++p) {
        in1[p] = fmaf(x.x, ca[p], in1[p]);
        in1[p] = fmaf(x.y, ca[p], in1[p]);
        in1[p] = fmaf(x.z, ca[p], in1[p]);
        in1[p] = fmaf(x.w, ca[p], in1[p]);
      }
    } else if (FAMILY == MI_NORMAL) {
#pragma unroll
      for (int p = 0; p < kBcastP; ++p) {
        const float d0 = x.x - ca[p], d1 = x.y - ca[p], d2 = x.z - ca[p], d3 = x.w - ca[p];
        if (MASKED || !exact) {
          const float e0 = y.x * d0, e1 = y.y * d1, e2 = y.z * d2, e3 = y.w * d3;
          in1[p] += (e0 + e1) + (e2 + e3);
          in2[p] = fmaf(e0, d0, fmaf(e1, d1, fmaf(e2, d2, fmaf(e3, d3, in2[p]))));
        } else {
          in1[p] += (d0 + d1) + (d2 + d3);
          in2[p] = fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, fmaf(d3, d3, in2[p]))));
        }
      }
    } else {
#pragma unroll
      for (int p = 0; p < kBcastP; ++p) {
        in1[p] = fmaf(x.x, ca[p], fmaf(x.y, ca[p], fmaf(x.z, ca[p], fmaf(x.w, ca[p], in1[p]))));
        in1[p] = fmaf(y.x, cb[p], fmaf(y.y, cb[p], fmaf(y.z, cb[p], fmaf(y.w, cb[p], in1[p]))));
      }
    }
  };

  const int nq = (int)((len + 3) / 4);
  const int full = (int)(len / 4) & ~15;
  if constexpr (FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS) {
    // x l summed over the chunk for 8 particles: packed FMAs (v_pk_fma_f32) on particle pairs,
    // two evals per lane per instruction. The zero padding of the last quad is neutral.
    f32x2 cav[kBcastP / 2];
#pragma unroll
    for (int j = 0; j < kBcastP / 2; ++j) cav[j] = f32x2{ca[2 * j], ca[2 * j + 1]};
    // feat[0][j] = (x_2j, x_2j, x_2j+1, x_2j+1); the chunk's zero padding is neutral.
    const int npair = (int)((len + 1) / 2);
    for (int j0 = 0; j0 < npair; j0 += 64) {
      // two accumulator sets (even / odd elements): 8 independent FMA chains per lane, flushed to
      // fp64 every 128 elements
      f32x2 in[2][kBcastP / 2];
#pragma unroll
      for (int j = 0; j < kBcastP / 2; ++j) in[0][j] = in[1][j] = f32x2{0.0f, 0.0f};
      if (j0 + 64 <= npair) {
#pragma unroll
        for (int h = 0; h < 8; ++h) {
          float4 xs[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) xs[j] = feat[0][j0 + 8 * h + j];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const f32x2 xa = f32x2{xs[j].x, xs[j].y}, xb = f32x2{xs[j].z, xs[j].w};
#pragma unroll
            for (int pp = 0; pp < kBcastP / 2; ++pp) {
              in[0][pp] = __builtin_elementwise_fma(xa, cav[pp], in[0][pp]);
              in[1][pp] = __builtin_elementwise_fma(xb, cav[pp], in[1][pp]);
            }
          }
        }
      } else {
        for (int j = j0; j < npair; ++j) {
          const float4 x = feat[0][j];
          const f32x2 xa = f32x2{x.x, x.y}, xb = f32x2{x.z, x.w};
#pragma unroll
          for (int pp = 0; pp < kBcastP / 2; ++pp) {
            in[0][pp] = __builtin_elementwise_fma(xa, cav[pp], in[0][pp]);
            in[1][pp] = __builtin_elementwise_fma(xb, cav[pp], in[1][pp]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kBcastP / 2; ++j) {
        const f32x2 t = in[0][j] + in[1][j];
        acc1[2 * j] += (double)t.x;
        acc1[2 * j + 1] += (double)t.y;
      }
    }
  } else {
  for (int q0 = 0; q0 < full; q0 += 16) {
    float in1[kBcastP], in2[kBcastP];
#pragma unroll
    for (int p = 0; p < kBcastP; ++p) in1[p] = in2[p] = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float4 xs[8], ys[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xs[j] = feat[0][q0 + 8 * h + j];
        ys[j] = NF > 1 ? feat[NF - 1][q0 + 8 * h + j] : xs[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) quad(xs[j], ys[j], in1, in2, true);
    }
#pragma unroll
    for (int p = 0; p < kBcastP; ++p) {
      acc1[p] += (double)in1[p];
      acc2[p] += (double)in2[p];
    }
  }
  {
    float in1[kBcastP], in2[kBcastP];
#pragma unroll
    for (int p = 0; p < kBcastP; ++p) in1[p] = in2[p] = 0.0f;
    for (int q = full; q < nq; ++q) {
      const float4 x = feat[0][q];
      const float4 y = NF > 1 ? feat[NF - 1][q] : x;
      quad(x, y, in1, in2, false);
    }
#pragma unroll
    for (int p = 0; p < kBcastP; ++p) {
      acc1[p] += (double)in1[p];
      acc2[p] += (double)in2[p];
    }
  }
  }

  // ---- epilogue: constant parts, gradients, partial writes -------------------------------------
  const int o_a = st.operand[0], o_b = st.operand[1];
  const bool grads = G.compute_grads != 0;
  const int slot_a = (grads && o_a >= 0 && G.operands[o_a].grad_mode == MI_GRAD_PARTICLE) ? G.operands[o_a].slot : -1;
  const int slot_b = (grads && o_b >= 0 && G.operands[o_b].grad_mode == MI_GRAD_PARTICLE) ? G.operands[o_b].slot : -1;
  const double M = s_m;
  const float w = (float)st.scale;
#pragma unroll
  for (int p = 0; p < kBcastP; ++p) {
    const int64_t k = kbase + p * kBcastThreads;
    double lp = 0.0;
    float ga = 0.0f, gb = 0.0f;
    const int64_t kc = min(k, K - 1);
    if (FAMILY == MI_BERNOULLI_LOGITS || FAMILY == MI_BERNOULLI_PROBS) {
      const double softplus = prep[2 * K + kc], sig = prep[3 * K + kc];
      lp = acc1[p] - M * softplus;
      ga = (float)(((double)s_a - M * sig) * (double)cb[p]);
    } else if (FAMILY == MI_NORMAL) {
      const double sigma = cb[p];
      const double inv2 = 1.0 / (sigma * sigma);
      lp = -0.5 * acc2[p] * inv2 - M * (double)prep[2 * K + kc];
      ga = (float)(acc1[p] * inv2);
      gb = (float)(acc2[p] * inv2 / sigma - M / sigma);
    } else {
      double base = acc1[p] + M * (double)prep[2 * K + kc];
      // xlogy semantics for exact 0 / 1 values (dirichlet.py:94)
      if (s_zero > 0.0f && ca[p] != 0.0f) base += ca[p] > 0.0f ? -__builtin_inf() : __builtin_inf();
      if (s_one > 0.0f && cb[p] != 0.0f) base += cb[p] > 0.0f ? -__builtin_inf() : __builtin_inf();
      lp = base;
      ga = (float)((double)s_a + M * (double)prep[3 * K + kc] -
                   (s_zero > 0.0f ? __builtin_inf() : 0.0));
      gb = (float)((double)s_b + M * (double)prep[4 * K + kc] -
                   (s_one > 0.0f ? __builtin_inf() : 0.0));
    }
    if (k < G.K) {
      part[((int64_t)0 * nchunk + c) * G.K + k] = (float)lp;
      if (slot_a >= 0) part[((int64_t)(1 + slot_a) * nchunk + c) * G.K + k] = w * ga;
      if (slot_b >= 0) part[((int64_t)(1 + slot_b) * nchunk + c) * G.K + k] = w * gb;
    }
  }
  publish_flags(flags, fl);
}

// Bernoulli BCAST over unmasked contiguous data, the shared values read by the scalar unit.
// Every lane of a wave needs the same x_i, so the chunk is read with s_load (constant address
// space, wave-uniform addresses) into SGPRs, and a v_pk_fma_f32 takes the SGPR pair (x_i, x_i+1)
// against the VGPR pair (l_k, l_k) of one particle: two evals per lane per instruction with no LDS
// traffic (the LDS kernel above moves 1 KB of broadcast data per 8 packed FMAs).
//
// log p(x | l) = x l - softplus(l) and d/dl = x - sigmoid(l), so a chunk's partials are
//   lp:   sum_i x_i l_k            slot: w dl_k sum_i x_i
// and the particle-constant parts, -N softplus(l_k) and -N w dl_k sigmoid(l_k), are written once,
// by the chunk-0 blocks, into one extra segment (index gridDim.x): no chunk repeats the
// transcendentals, and k_finalize adds the extra segment like any other (nseg = chunks + 1).
// Partial sums: fp32 over at most 64 terms (as k_site_bcast), carried in fp64.
typedef const __attribute__((address_space(4))) float smem_float;

// One workgroup of a group's side job (mi_side): the mi_beta_dgrad factors of 256 (draw, component)
// pairs, one per thread -- latency-bound fp64 chains that run beside the site workgroups.
MI_DEV void beta_side_block(const mi_side& S, int64_t b) {
  const int64_t t = b * kBcastThreads + threadIdx.x;
  if (t >= 2 * S.K * S.N) return;
  const int j = (int)(t & 1);
  const int64_t e = t >> 1, i = e % S.N;
  const float a = S.c1[i * S.c1_stride], bb = S.c0[i * S.c0_stride];
  const float tot = a + bb;  // concentration.sum(-1) in fp32, dirichlet.py:18
  const double psi_t = digamma((double)tot);
  const float xv = S.x[e];
  S.out[t] = (
                   j == 0 ? dirichlet_grad(xv, a, tot, digamma((double)a), psi_t) * (double)(1.0f - xv)
                          : -dirichlet_grad(1.0f - xv, bb, tot, digamma((double)bb), psi_t) * (double)xv);
}


// Grid (1-D): gy particle blocks of each chunk, chunks padded to a multiple of 8, dealt so that
// every particle block of chunk c runs on the same XCD (workgroups go to the 8 XCDs round-robin:
// block b -> XCD b % 8 = c % 8) and the chunk is fetched into that XCD's L2 once; then the side
// job's workgroups.
// rank1: the slot value is written in the rank-one layout of mi_reduce.rank1 (the chunk sums u[c]
// from the particle-block-0 workgroups, f[k] = w dl_k and e[k] = -N w sigmoid(l_k) dl_k from the
// chunk-0 workgroups) instead of one partial per (chunk, particle): half the partial slab.
// SUFF (MININF_AMD_BCAST_SUFFSTAT=1, a measurement of the floor, not the default): the
// per-(particle, element) FMA loop replaced by its closed form l_k * sum_i x_i -- the same value
// in exact arithmetic (C2's per-eval arithmetic is reducible).
// ksum (mode bit 2, MI_GROUP_KSUM): the site value leaves the launch summed over the workgroup's
// particles (mi_reduce.ksum) -- registers, then wave, then LDS, in fp64 and a fixed order -- as one
// double per workgroup, ksum[c * gy + particle block], and the particle-constant segment as one
// more from each workgroup that evaluates it, ksum[(chunks + s) * gy + particle block] (s: the
// particle slot, 0 when chunk 0 takes them all). Lanes past K add exactly zero. No [nseg, K] value
// block exists then: `part` starts with the slot's block.
// chunk: elements per chunk, a multiple of 32 and at most kSmemMaxChunk (the host sizes it so that
// chunks x particle blocks fill the chip's workgroup slots: make_plan).

// The timeline build (tools/c2_timeline.py compiles this file with MI_SITES_TIMELINE defined):
// thread 0 of every workgroup of k_site_bcast_smem records the constant-rate clock (s_memrealtime,
// 100 MHz) at entry (0), after the logits (1), after the chunk pass and its barrier round (2),
// after the last read-out of the first matrix pass (3), after the matrix loop (4), after the
// chunks' values are stored (5) and at exit (6), into row blockIdx.x of g_tl; word 7 is
// kind + 2 (particle block + 16 chunk group), kind 1 for a side-job workgroup.
#ifdef MI_SITES_TIMELINE
constexpr int kTimelineRows = 8192;
__device__ unsigned long long g_tl[kTimelineRows * 8];
#define MI_TL_BEGIN() \
  unsigned long long tl_[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull}; \
  tl_[0] = __builtin_amdgcn_s_memrealtime()
#define MI_TL(i) tl_[i] = __builtin_amdgcn_s_memrealtime()
#define MI_TL_END(kind, group, kb) \
  do { \
    __syncthreads(); \
    if (threadIdx.x == 0 && blockIdx.x < kTimelineRows) { \
      unsigned long long* row_ = g_tl + (size_t)blockIdx.x * 8; \
      for (int i_ = 0; i_ < 6; ++i_) row_[i_] = tl_[i_]; \
      row_[6] = __builtin_amdgcn_s_memrealtime(); \
      row_[7] = (unsigned long long)(kind) + 2ull * ((unsigned long long)(kb) + 16ull * (unsigned long long)(group)); \
    } \
  } while (0)
#else
#define MI_TL_BEGIN() do {} while (0)
#define MI_TL(i) do {} while (0)
#define MI_TL_END(kind, group, kb) do {} while (0)
#endif

// The matrix loop of k_site_bcast_smem (mode bit 3, MININF_AMD_BCAST_MFMA): a chunk whose elements
// are all exactly 0 or 1 is summed on the int8 matrix cores with no rounding anywhere.
//   * x_i in {0, 1} is exact in int8.
//   * a finite fp32 logit with sign s, biased exponent e and fraction f is (-1)^s M 2^E exactly,
//     M = f + (e > 0 ? 2^23 : 0) its significand and E = max(e, 1) - 150 (subnormals and zeros
//     included: nothing is lost below any format's normal range). With c = (e > 0 ? 2^23 : 0) + 2^22
//     the rest r = M - c = f - 2^22 lies in [-2^22, 2^22) and is three balanced base-256 digits,
//     r = d0 + 256 d1 + 65536 d2, each in [-128, 127]: three int8 pieces.
//   * every accumulator element is (a count <= 4096) x (one digit), |.| <= 2^19, exact in int32 in
//     any order; each digit keeps accumulators of its own. With n1 the chunk's count of ones,
//     S = c n1 + D0 + 256 D1 + 65536 D2 = M n1 (< 2^36, int64) and the chunk's total is
//     (-1)^s S 2^E in fp64, a power-of-two scale: l_k sum_i x_i exactly.
// Every eval is still its own multiply-accumulate, x_i times a digit of l_k, but on the 23 fraction
// bits recentred by 2^22 only: the implicit leading one and the recentring constant, c, are the same
// for every element and enter once per (chunk, particle) through the count of ones, which the
// kernel has as the chunk sum it forms for the gradient.
// D = A B with v_mfma_i32_16x16x64_i8: A[row][k] holds 1024 consecutive elements of the staged
// chunk (any element may sit in any slot: B is constant over k and all of D's rows are added up at
// the end, so only the C/D lane map is used), B[k][col] is the digit of the tile's particle `col`
// in every k. A wave takes the 4 x 64 particles its lanes own in passes of kMatrixP particles per
// lane: 4 column tiles x 3 digits per particle slot, each with a 4-register accumulator and a
// 4-register B fragment. One chunk per workgroup: kMatrixP = 2 slots a pass, 2 x 4 x 3 x (4 + 4) =
// 192 registers and 24 instructions per fragment, two waves per SIMD (all four slots in one pass
// take 384: one wave per SIMD). Several chunks per workgroup: one slot a pass, 96 registers and 12
// instructions per fragment, three waves per SIMD (the digits stay live across a chunk's read-out).
typedef int i32x4 __attribute__((ext_vector_type(4)));   // a fragment, or an accumulator, as its four registers
constexpr int kMatrixP = 2;
constexpr int kFragElems = 1024;   // elements per A fragment: 16 rows x 64 k

// The three digits of a logit's recentred fraction, each as its byte repeated over a B fragment's
// sixteen k. (A non-finite logit gets digits too; its total is made on the vector side.)
MI_DEV void logit_pieces(float l, i32x4 (&b)[3]) {
  int r = (int)(__builtin_bit_cast(uint32_t, l) & 0x7fffffu) - (1 << 22);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int d = ((r & 0xff) ^ 0x80) - 0x80;   // the balanced digit: r's low byte, signed
    r = (r - d) >> 8;                           // (exact: r - d is a multiple of 256)
    const int vv = (d & 0xff) * 0x01010101;
    b[q] = i32x4{vv, vv, vv, vv};
  }
}

// l n1 from the digit sums D of one (chunk, particle): (-1)^s (c n1 + D0 + 256 D1 + 65536 D2) 2^E,
// exact in fp64 (a zero total is +0, as a sum from 0.0 is). A non-finite logit: l n1, non-finite.
MI_DEV double logit_total(float l, int n1, const int (&D)[3]) {
  const uint32_t u = __builtin_bit_cast(uint32_t, l);
  const int e = (int)((u >> 23) & 0xffu);
  if (e == 0xff) return (double)l * (double)n1;   // (an infinity over no ones: NaN)
  const int64_t c = (e > 0 ? (int64_t)1 << 23 : 0) + ((int64_t)1 << 22);
  const int64_t S = c * n1 + D[0] + 256 * (int64_t)D[1] + 65536 * (int64_t)D[2];
  const double scale = __builtin_bit_cast(double, (uint64_t)(max(e, 1) - 150 + 1023) << 52);
  return (double)((u >> 31) != 0u ? -S : S) * scale;
}

// sum_i x_i l_k for the kSmemP particles of every lane, for each of the workgroup's chunks whose bit
// is set in `mat`: chunk j staged at xa + j kSmemMaxChunk as int8 (zeros past its end, up to a whole
// fragment), nfrag(j) >= 1 fragments long, ones(j) of its elements a one. The digits of a pass are
// split once and every chunk walks them; a chunk's accumulators are read out before the next chunk
// starts (each chunk keeps a partial of its own), and `fold(j, p, total)` takes the total of chunk j
// and particle slot p: slots in order within a chunk. `first_k`: the wave's first particle of slot 0.
template <int kSmemP, int CPW, int MP, typename Frags, typename Ones, typename Fold>
MI_DEV void bcast_matrix_loop(const signed char* xa, uint32_t mat, Frags nfrag, Ones ones,
                              const f32x2 (&ld)[kSmemP], int64_t first_k, int64_t K, Fold fold) {
  static_assert(kSmemP % MP == 0, "whole passes");
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, grp = lane >> 4;
#pragma unroll
  for (int p0 = 0; p0 < kSmemP; p0 += MP) {
    // (wave-uniform: a pass none of whose particles exist is skipped; its lanes store nothing)
    if (first_k + (int64_t)p0 * kBcastThreads >= K) continue;
    i32x4 b[MP][4][3];
#pragma unroll
    for (int pp = 0; pp < MP; ++pp)
#pragma unroll
      for (int g = 0; g < 4; ++g) logit_pieces(__shfl(ld[p0 + pp].x, g * 16 + col, 64), b[pp][g]);
    // (not unrolled: one copy of the loop, and the registers of one chunk, whatever CPW is)
#pragma unroll 1
    for (int j = 0; j < CPW; ++j) {
      if (((mat >> j) & 1u) == 0u) continue;   // (uniform over the workgroup)
      const i32x4* frag = reinterpret_cast<const i32x4*>(xa + j * kSmemMaxChunk) + lane;
      const int nf = nfrag(j);
      const int n1 = ones(j);
      i32x4 d[MP][4][3];
#pragma unroll
      for (int pp = 0; pp < MP; ++pp)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int q = 0; q < 3; ++q) d[pp][g][q] = i32x4{0, 0, 0, 0};
      // The loop is written out: from the builtin the compiler routes half the accumulators through
      // a scratch tile, four register moves and a wait per instruction. Accumulators are tied in
      // AGPRs, fragments stay in VGPRs; between two instructions on one accumulator stand 23 others
      // (11 with one slot a pass).
      // The compiler's hazard recogniser does not see inside the assembly: after a toolchain change
      // read the ISA of this loop again (the accumulators' zeroing before the first instruction,
      // the s_waitcnt before the fragment's first use, the waits after the loop).
      int f = 0;
      i32x4 next = frag[0];
      do {   // (nf >= 1: a chunk is never empty. The next fragment's read is issued ahead of
             // this fragment's 24 (or 12) instructions and waited for behind them: one iteration of overlap,
             // not a second buffer.)
        const i32x4 a = next;
        next = frag[min(f + 1, nf - 1) * (kFragElems / 16)];
#pragma unroll
        for (int pp = 0; pp < MP; ++pp)
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 3; ++q)
              __asm__ volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0"
                               : "+a"(d[pp][g][q]) : "v"(a), "v"(b[pp][g][q]));
      } while (++f < nf);
      // v_mfma_i32_16x16x64_i8 is an 8-pass instruction, and a VALU read of a matrix result
      // has to stand passes + 3 = 11 wait states behind it (19 behind a 16-pass one; the compiler's
      // hazard table for gfx950). Each statement below waits 32 (two s_nop 15); there are MP
      // of them, in order, each tied to half the accumulators. They stand before every read-out:
      // once per chunk and pass.
#pragma unroll
      for (int pp = 0; pp < MP; ++pp)
        __asm__ volatile("s_nop 15\n\ts_nop 15"
                         : "+a"(d[pp][0][0]), "+a"(d[pp][0][1]), "+a"(d[pp][0][2]), "+a"(d[pp][1][0]),
                           "+a"(d[pp][1][1]), "+a"(d[pp][1][2]), "+a"(d[pp][2][0]), "+a"(d[pp][2][1]),
                           "+a"(d[pp][2][2]), "+a"(d[pp][3][0]), "+a"(d[pp][3][1]), "+a"(d[pp][3][2]));
      // D's rows: four registers, then the four lane groups. Lane group g keeps tile g (its lanes
      // own that tile's particles), so the groups trade halves instead of all summing every tile.
      // (int32, exact: count x digit.) The lane then owns the digit sums of its own particle.
#pragma unroll
      for (int pp = 0; pp < MP; ++pp) {
        int D[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          int v[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            v[g] = (d[pp][g][q].x + d[pp][g][q].y) + (d[pp][g][q].z + d[pp][g][q].w);
          }
          const bool hi = grp >= 2, odd = (grp & 1) != 0;
          const int w0 = (hi ? v[2] : v[0]) + __shfl_xor(hi ? v[0] : v[2], 32, 64);
          const int w1 = (hi ? v[3] : v[1]) + __shfl_xor(hi ? v[1] : v[3], 32, 64);
          D[q] = (odd ? w1 : w0) + __shfl_xor(odd ? w0 : w1, 16, 64);
        }
        fold(j, p0 + pp, logit_total(ld[p0 + pp].x, n1, D));
      }
    }
  }
}

// MATRIX: the instantiation that holds the matrix loop (236 / 232 registers with 96 AGPRs and 4 KB
// of LDS: two waves per SIMD). Without it the kernel is the scalar-load loop alone, at its 90
// registers and four workgroups per CU: what MININF_AMD_BCAST_MFMA=0 launches.
// (CPW = 2 / 4: one particle slot per matrix pass, 152 / 148 registers with 48 AGPRs, 12 / 24 KB
// of LDS, no scratch: three waves per SIMD.)
// CPW (chunks per workgroup, the matrix instantiation only; MININF_AMD_BCAST_CPW): the workgroup
// owns particle block `kblock` and the CPW consecutive chunks of chunk group g, [g CPW, min((g + 1)
// CPW, chunks)). The chunk plan, every partial and every index written are those of CPW = 1; what
// is paid once per workgroup instead of once per chunk is the setup (arguments, parameters, logits),
// the latency of the chunk pass (all the group's loads are in flight together), one barrier round
// for all the chunk sums and flags, the digit splits of a pass and the slot epilogue. launch_smem
// picks CPW so that the grid fits one round of resident workgroups. With CPW > 1 the side job's
// workgroups (padded to a multiple of 8: the XCD mapping stays) come first in the grid.
template <int FAMILY, int kSmemP, bool SUFF = false, bool MATRIX = false, int CPW = 1>
__global__ __launch_bounds__(kBcastThreads) void k_site_bcast_smem(const mi_group G,
                                                                   float* __restrict__ part,
                                                                   int64_t nseg, int gy,
                                                                   int mode, int chunk,
                                                                   uint32_t* __restrict__ flags,
                                                                   double* __restrict__ ksum) {
  static_assert(CPW == 1 || (MATRIX && !SUFF), "several chunks per workgroup: the matrix loop only");
  static_assert(CPW >= 1 && CPW <= 4, "the staged chunks: at most 16 KB of LDS");
  constexpr int kWaves = kBcastThreads / 64;
  __shared__ float scratch[CPW * kWaves];
  __shared__ double dscratch[CPW * kWaves];
  __shared__ uint32_t other_of_wave[kWaves];
  __shared__ double lane_sum[CPW > 1 ? CPW * kBcastThreads : 1];   // (below: the matrix loop's fold)
  __shared__ __attribute__((aligned(16))) signed char xa[MATRIX ? CPW * kSmemMaxChunk : 16];   // the matrix loop's chunks
  kernarg_prefetch<(int)sizeof(mi_group)>();
  MI_TL_BEGIN();
  // mode bit 0: rank-one slot layout; bit 1: progress-balanced wave priority (below); bit 2:
  // particle-summed values
  const int rank1 = mode & 1;
  const bool balance = (mode & 2) != 0;
  const bool ksummed = (mode & 4) != 0;
  constexpr bool try_matrix = MATRIX && !SUFF;
  const int64_t chunks = nseg - 1;
  const int64_t groups = (chunks + CPW - 1) / CPW;
  const int64_t padded = (groups + 7) / 8 * 8;
  int64_t b = blockIdx.x;
  // The side job (mi_side): the workgroups past the chunks, or (CPW > 1) those before them, so that
  // they start with the launch and the main workgroups that wait for their slots start within the
  // side job's length.
  // (their number from the arguments, as make_plan counts them: gridDim is a load from a line of
  // the argument segment that nothing has prefetched, in front of every workgroup)
  const int64_t side = (beta_side_blocks(G.side) + 7) / 8 * 8;
  if (CPW == 1 ? b >= padded * gy : b < side) {
    const unsigned long long ts = span_begin(G.stamps);   // (the launch's span includes them)
    beta_side_block(G.side, CPW == 1 ? b - padded * gy : b);   // (padding: past the job's end)
    span_end(G.stamps, ts);
    MI_TL_END(1, 0, 0);
    return;
  }
  if (CPW > 1) b -= side;
  const int64_t g = (b / (8 * gy)) * 8 + b % 8;
  const int64_t kblock = (b / 8) % gy;
  if (g >= groups) return;   // padding
  const unsigned long long t0 = span_begin(G.stamps);
  const mi_site& st = G.sites[0];
  const float* xg = G.operands[st.operand[2]].data;
  const int64_t c0 = g * CPW;   // the workgroup's chunks: c0 + j, j < nc
  const int nc = (int)min((int64_t)CPW, chunks - c0);
  // (pinned: a reload of N inside the matrix loop would be a scalar load among its LDS reads, and
  // the fragment prefetch would then be waited for at once)
  const int64_t left = CPW > 1 ? pin(G.N - c0 * chunk) : G.N - c0 * chunk;
  auto chunk_len = [&](int j) -> int {
    return j < nc ? (int)min((int64_t)chunk, left - (int64_t)j * chunk) : 0;
  };
  uint32_t fl = 0u;

  // ---- per-particle logits (as k_bcast_prep) ---------------------------------------------------
  // Only the logits live through the FMA loop (as the duplicated pairs ld): d l / d theta is
  // computed again after it, from the same values by the same code (r06: 102 -> 78 VGPR with the
  // particle-constant segment below; 86.2 vs 87.6 us per C2 step, profiles/r06_ab.json ab14).
  const int64_t K = G.K;
  const int64_t kbase = kblock * (kBcastThreads * kSmemP) + threadIdx.x;
  auto logits = [&](int p, float& l, float& d) -> bool {
    const int64_t k = kbase + p * kBcastThreads;
    const float a = role_scalar(G, st, 0, min(k, K - 1));
    d = 1.0f;
    if (FAMILY == MI_BERNOULLI_PROBS) {
      bernoulli_probs_to_logits(a, l, d);
      return !(a >= 0.0f && a <= 1.0f);
    }
    l = a;
    return a != a;
  };
  f32x2 ld[kSmemP];
#pragma unroll
  for (int p = 0; p < kSmemP; ++p) {
    float l, d;
    const bool bad = logits(p, l, d);
    ld[p] = f32x2{l, l};
    fl |= (g == 0 && kbase + p * kBcastThreads < K && bad) ? MI_FLAG_PARAM : 0u;
  }
  MI_TL(1);

  // ---- chunk sums and support flags (vector loads) ---------------------------------------------
  // Each lane takes kSmemMaxChunk / kBcastThreads consecutive elements of every chunk (those within
  // it) with all its loads, of all the workgroup's chunks, in flight at once (a strided loop waits
  // for one L2 round trip per element group, at the end of every wave). STAGE: the lane's elements
  // also go to `xa` as int8 (one 16-byte write), zeros past the chunk's end. A chunk's sum adds the lane's elements in
  // order from 0, then block_sum's tree: the same bits whatever CPW is.
  constexpr int kPerLane = kSmemMaxChunk / kBcastThreads;
  static_assert(kPerLane == 16, "whole float4 groups, and one 16-byte int8 group, per lane");
  float s_a[CPW];
  uint32_t other = 0u;   // bit j: one of this lane's elements of chunk j is neither 0 nor 1
  auto chunk_pass = [&](auto stage_tag) {
    constexpr bool STAGE = decltype(stage_tag)::value && MATRIX;
    const int e0 = (int)threadIdx.x * kPerLane;
    float4 t[CPW][kPerLane / 4];
    bool whole[CPW];
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const float* xl = xg + (c0 + j) * chunk + e0;
      whole[j] = e0 + kPerLane <= chunk_len(j) && (reinterpret_cast<uintptr_t>(xl) & 15) == 0;
      if (whole[j]) {
#pragma unroll
        for (int q = 0; q < kPerLane / 4; ++q) t[j][q] = reinterpret_cast<const float4*>(xl)[q];
      }
    }
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int len = chunk_len(j);
      signed char* xj = xa + (STAGE ? j * kSmemMaxChunk : 0);
      float s = 0.0f;
      bool bad = false;
      if (whole[j]) {
        float v[kPerLane];
#pragma unroll
        for (int q = 0; q < kPerLane / 4; ++q) {
          v[4 * q] = t[j][q].x;
          v[4 * q + 1] = t[j][q].y;
          v[4 * q + 2] = t[j][q].z;
          v[4 * q + 3] = t[j][q].w;
        }
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) {
          bad |= !(v[e] == 0.0f || v[e] == 1.0f);
          s += v[e];
        }
        if (STAGE) {
          // (1.0f's lowest exponent bit, set, is the int8 one; a chunk with any other value is not
          // read from the image)
          i32x4 h;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t w = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              w |= ((__builtin_bit_cast(uint32_t, v[4 * q + e]) >> 23) & 1u) << (8 * e);
            h[q] = (int)w;
          }
          *reinterpret_cast<i32x4*>(xj + e0) = h;
        }
      } else if (j < nc) {
        const float* xc = xg + (c0 + j) * chunk;
#pragma unroll 1
        for (int e = e0; e < len && e < e0 + kPerLane; ++e) {
          const float x = xc[e];
          bad |= !(x == 0.0f || x == 1.0f);
          s += x;
          if (STAGE) xj[e] = x == 1.0f ? 1 : 0;
        }
        if (STAGE)
          for (int e = max(e0, len); e < e0 + kPerLane; ++e) xj[e] = 0;
      }
      s_a[j] = s;
      other |= bad ? 1u << j : 0u;
    }
    fl |= other != 0u ? MI_FLAG_SUPPORT : 0u;
  };

  // ---- partials of a chunk's site value ------------------------------------------------------
  const int64_t first_k = kblock * (kBcastThreads * kSmemP) + (threadIdx.x & ~63);
  auto store_values = [&](int64_t c, const double (&acc)[kSmemP]) {
    double vsum = 0.0;
#pragma unroll
    for (int p = 0; p < kSmemP; ++p) {
      const int64_t k = kbase + p * kBcastThreads;
      if (k >= K) continue;
      if (ksummed) vsum += acc[p];
      else part[c * K + k] = (float)acc[p];
    }
    if (ksummed) {
      vsum = block_sum(vsum, dscratch);
      if (threadIdx.x == 0) ksum[c * gy + kblock] = vsum;
    }
  };

  // The matrix loop needs a whole chunk to be 0/1, so with it enabled the pass runs first: it
  // stages the chunks, and the workgroup agrees on the answer for each of them in one barrier round
  // (the chunk sums' round; wave-uniform, no host round trip).
  uint32_t scalar_chunks = (1u << nc) - 1u;   // bit j: chunk j takes the scalar-load loop
  if constexpr (try_matrix) {
    chunk_pass(std::true_type{});
    uint32_t any = other;
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) any |= __shfl_xor(any, offset, kWave);
    if ((threadIdx.x & 63) == 0) other_of_wave[threadIdx.x >> 6] = any;
    block_sum_n<CPW>(s_a, scratch);   // (its barriers publish other_of_wave and the staged chunks)
    any = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) any |= other_of_wave[w];
    scalar_chunks &= any;
    MI_TL(2);
    const uint32_t mat = ((1u << nc) - 1u) & ~any;
    if (mat != 0u) {
      // A chunk's particle sum in the present order: slots 0, 1 from the first pass, 2, 3 from the
      // second, from 0.0, lanes past K adding nothing. No per-slot totals live through the loop:
      // the lane's running sum of chunk j is a register (CPW = 1) or its own LDS word.
      // Particle slots per pass: kMatrixP, or one where the digits have to stay live through a
      // chunk's read-out for the next chunk (CPW > 1: 48 + 48 registers a pass instead of 96 + 96,
      // the chunk read from LDS four times instead of twice).
      constexpr int kPassP = CPW > 1 ? 1 : kMatrixP;
      double vsum[CPW];
#pragma unroll
      for (int j = 0; j < CPW; ++j) vsum[j] = 0.0;
      if constexpr (CPW > 1) {
#pragma unroll
        for (int j = 0; j < CPW; ++j) lane_sum[j * kBcastThreads + threadIdx.x] = 0.0;
      }
      // (a 0/1 chunk's sum is its count of ones, exact and at most 4096; 16 bits each of one word,
      // so that the loop over the chunks indexes no array. A chunk with any other value has a sum
      // of any size or sign, or none: its field stays zero and is never read.)
      uint64_t ones = 0u;
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const float n1 = ((mat >> j) & 1u) != 0u ? s_a[j] : 0.0f;
        ones |= (uint64_t)((uint32_t)n1 & 0xffffu) << (16 * j);
      }
      bcast_matrix_loop<kSmemP, CPW, kPassP>(
          xa, mat, [&](int j) { return (chunk_len(j) + kFragElems - 1) / kFragElems; },
          [&](int j) { return (int)((ones >> (16 * j)) & 0xffffu); },
          ld, first_k, K,
          [&](int j, int p, double total) {
            const int64_t k = kbase + p * kBcastThreads;
            if (p == kPassP - 1) MI_TL(3);
            if (k >= K) return;
            if (!ksummed) part[(c0 + j) * K + k] = (float)total;
            else if constexpr (CPW == 1) vsum[0] += total;
            else lane_sum[j * kBcastThreads + threadIdx.x] += total;
          });
      MI_TL(4);
      if (ksummed) {
        if constexpr (CPW > 1) {
#pragma unroll
          for (int j = 0; j < CPW; ++j) vsum[j] = lane_sum[j * kBcastThreads + threadIdx.x];
        }
        block_sum_n<CPW>(vsum, dscratch);
        if (threadIdx.x == 0) {
#pragma unroll
          for (int j = 0; j < CPW; ++j)
            if ((mat >> j) & 1u) ksum[(c0 + j) * gy + kblock] = vsum[j];
        }
      }
    }
  }
  MI_TL(5);

  // ---- sum_i x_i l_k: element pairs from SGPRs against duplicated particle logits --------------
  // (a chunk with any other value, and every chunk with the matrix loop off: the scalar-load loop,
  // one chunk at a time)
#pragma unroll 1
  for (int cj = 0; cj < (try_matrix ? nc : 1); ++cj) {
    if constexpr (try_matrix)
      if (((scalar_chunks >> cj) & 1u) == 0u) continue;
    double acc[kSmemP];
#pragma unroll
    for (int p = 0; p < kSmemP; ++p) acc[p] = 0.0;
    const int64_t i0 = (c0 + cj) * chunk;
    const int vlen = chunk_len(cj);
    smem_float* xs = (smem_float*)(xg + i0);
    auto flush = [&](const f32x2 (&in)[2][kSmemP]) {
#pragma unroll
      for (int p = 0; p < kSmemP; ++p)
        acc[p] += (double)((in[0][p].x + in[0][p].y) + (in[1][p].x + in[1][p].y));
    };
    // Whole 256-element blocks in groups of 32 (two s_load_dwordx16): the next group's loads are in
    // flight during this group's packed FMAs (scalar loads return out of order, so every use waits
    // for all of them: one group of lookahead). Even and odd element pairs go to separate
    // accumulators, 2 kSmemP independent chains of 64 terms per block.
    constexpr int kGroup = 32, kBlock = 256;
    const int nfull = SUFF ? 0 : vlen & ~(kBlock - 1);
    int j = 0;
    if (nfull > 0) {
      float xc[kGroup];
#pragma unroll
      for (int e = 0; e < kGroup; ++e) xc[e] = xs[e];
      // the first block index of each later quarter of the chunk (no division inside the loop)
      const int q1 = (nfull / 4 + kBlock - 1) & ~(kBlock - 1), q2 = (nfull / 2 + kBlock - 1) & ~(kBlock - 1),
                q3 = (3 * nfull / 4 + kBlock - 1) & ~(kBlock - 1);
      if (balance) __builtin_amdgcn_s_setprio(3);
      for (; j < nfull; j += kBlock) {
        // Progress-balanced priority: a wave drops one priority level per quarter of its chunk, so
        // the SIMD's arbiter (priority, then age) lets the waves behind it catch up; the waves of a
        // SIMD then finish together instead of the oldest first, which would leave the last one
        // issuing alone (at half the VALU rate) through the kernel's tail.
        if (balance) {
          if (j == q1) __builtin_amdgcn_s_setprio(2);
          else if (j == q2) __builtin_amdgcn_s_setprio(1);
          else if (j == q3) __builtin_amdgcn_s_setprio(0);
        }
        f32x2 in[2][kSmemP];
#pragma unroll
        for (int p = 0; p < kSmemP; ++p) in[0][p] = in[1][p] = f32x2{0.0f, 0.0f};
#pragma unroll
        for (int g = 0; g < kBlock; g += kGroup) {
          const int nxt = min(j + g + kGroup, nfull - kGroup);   // in bounds; the last is unused
          float xn[kGroup];
#pragma unroll
          for (int e = 0; e < kGroup; ++e) xn[e] = xs[nxt + e];
#pragma unroll
          for (int e = 0; e < kGroup; e += 2) {
            const f32x2 xv = f32x2{xc[e], xc[e + 1]};
#pragma unroll
            for (int p = 0; p < kSmemP; ++p)
              in[(e >> 1) & 1][p] = __builtin_elementwise_fma(xv, ld[p], in[(e >> 1) & 1][p]);
          }
#pragma unroll
          for (int e = 0; e < kGroup; ++e) xc[e] = xn[e];
        }
        flush(in);
      }
    }
    if (!SUFF && j + kGroup <= vlen) {   // whole groups of 32 past the last whole block
      f32x2 in[2][kSmemP];
#pragma unroll
      for (int p = 0; p < kSmemP; ++p) in[0][p] = in[1][p] = f32x2{0.0f, 0.0f};
      float xc[kGroup];
#pragma unroll
      for (int e = 0; e < kGroup; ++e) xc[e] = xs[j + e];
      for (; j + kGroup <= vlen; j += kGroup) {
        const int nxt = min(j + kGroup, vlen - kGroup);   // in bounds; the last is unused
        float xn[kGroup];
#pragma unroll
        for (int e = 0; e < kGroup; ++e) xn[e] = xs[nxt + e];
#pragma unroll
        for (int e = 0; e < kGroup; e += 2) {
          const f32x2 xv = f32x2{xc[e], xc[e + 1]};
#pragma unroll
          for (int p = 0; p < kSmemP; ++p)
            in[(e >> 1) & 1][p] = __builtin_elementwise_fma(xv, ld[p], in[(e >> 1) & 1][p]);
        }
#pragma unroll
        for (int e = 0; e < kGroup; ++e) xc[e] = xn[e];
      }
      flush(in);
    }
    if (!SUFF && j < vlen) {   // the chunk's tail: element pairs, a zero for an odd last element
      f32x2 in[2][kSmemP];
#pragma unroll
      for (int p = 0; p < kSmemP; ++p) in[0][p] = in[1][p] = f32x2{0.0f, 0.0f};
      for (int e = 0; j < vlen; j += 2, ++e) {
        const f32x2 xv = f32x2{xs[j], j + 1 < vlen ? xs[j + 1] : 0.0f};
#pragma unroll
        for (int p = 0; p < kSmemP; ++p)
          in[e & 1][p] = __builtin_elementwise_fma(xv, ld[p], in[e & 1][p]);
      }
      flush(in);
    }

    // (without the matrix loop the pass runs here, where the chunk is L2-resident)
    if (!try_matrix) {
      chunk_pass(std::false_type{});
      s_a[0] = block_sum(s_a[0], scratch);
    }
    if (SUFF) {
#pragma unroll
      for (int p = 0; p < kSmemP; ++p) acc[p] = (double)ld[p].x * (double)s_a[0];
    }
    store_values(c0 + cj, acc);
  }
  __asm__ volatile("" ::: "memory");   // (the parameters are read again, not held in registers)
  float dl[kSmemP];
#pragma unroll
  for (int p = 0; p < kSmemP; ++p) {
    float l;
    (void)logits(p, l, dl[p]);
  }

  // ---- partials of this chunk, and the particle-constant segment (below) --------------------
  const int o_a = st.operand[0];
  const int slot_a = (G.compute_grads != 0 && o_a >= 0 && G.operands[o_a].grad_mode == MI_GRAD_PARTICLE)
                         ? G.operands[o_a].slot : -1;
  const float w = (float)st.scale;
  const int64_t extra = nseg - 1;
  uint32_t fl_prior = 0u;
  float* slot_part = part + (int64_t)((ksummed ? 0 : 1) + slot_a) * nseg * K;   // (slot_a >= 0)
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    if (j >= nc) break;
    const int64_t c = c0 + j;
    if (rank1 && slot_a >= 0 && kblock == 0 && threadIdx.x == 0) slot_part[c] = s_a[j];   // u[c]
#pragma unroll
    for (int p = 0; p < kSmemP; ++p) {
      const int64_t k = kbase + p * kBcastThreads;
      if (k >= K) continue;
      if (slot_a >= 0 && !rank1) slot_part[c * K + k] = w * (s_a[j] * dl[p]);
    }
  }
  // The particle-constant segment: particle slot p of every lane by the workgroups of chunk group p
  // (group 0 takes all of them when the grid has fewer groups than particles per lane), one
  // particle at a time -- the prior's special functions interleaved over the particles held ~40
  // registers. The particle sums keep the layout of CPW = 1: one double per slot from four chunks
  // on (`spread`), one for all slots below that.
  const bool spread = chunks >= kSmemP;
  const bool dealt = groups >= kSmemP;
  if (dealt ? g < kSmemP : g == 0) {
    const int p0 = dealt ? (int)g : 0, p1 = dealt ? (int)g + 1 : kSmemP;
    double csum = 0.0;
#pragma unroll 1
    for (int p = p0; p < p1; ++p) {
      const int64_t k = kbase + p * kBcastThreads;
      if (k < K) {
        float l, dlp;
        (void)logits(p, l, dlp);
        const float t = expf(-fabsf(l));
        const double softplus = (double)(fmaxf(l, 0.0f) + log1pf(t));
        const double sig = (double)(l >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t));
        const double n = (double)G.N;
        // the folded prior site (mi_prior): log p(a_k) and d/da_k of the per-particle parameter a_k
        float prior_lp = 0.0f, prior_d = 0.0f;
        if (G.prior.present != 0) {
          const float a = role_scalar(G, st, 0, k);
          Elem pe;
          if (G.prior.family == MI_BETA) eval_beta(G.prior.constant[0], G.prior.constant[1], a, pe);
          else if (G.prior.family == MI_NORMAL) eval_normal(G.prior.constant[0], G.prior.constant[1], a, pe);
          else eval_gamma(G.prior.constant[0], G.prior.constant[1], a, pe);
          prior_lp = pe.lp;
          prior_d = pe.d[2];
          fl_prior |= (pe.param_bad ? MI_FLAG_PARAM : 0u) | (pe.support_bad ? MI_FLAG_SUPPORT : 0u);
        }
        const float cv = (float)(-n * softplus) + prior_lp;
        if (ksummed) csum += (double)cv;
        else part[extra * K + k] = cv;
        if (slot_a >= 0) {
          const float e = w * (float)(-n * sig * (double)dlp) + w * prior_d;
          if (rank1) {
            slot_part[nseg + k] = w * dlp;         // f[k]
            slot_part[nseg + K + k] = e;           // e[k]
          } else {
            slot_part[extra * K + k] = e;
          }
        }
      }
      if (ksummed && spread) {   // (uniform over the workgroup, as the loop's bounds)
        csum = block_sum(csum, dscratch);
        if (threadIdx.x == 0) ksum[(chunks + p) * gy + kblock] = csum;
        csum = 0.0;
      }
    }
    if (ksummed && !spread) {
      csum = block_sum(csum, dscratch);
      if (threadIdx.x == 0) ksum[chunks * gy + kblock] = csum;
    }
  }
  if (rank1 && slot_a >= 0 && kblock == 0 && threadIdx.x == 0 && g == 0) slot_part[extra] = 0.0f;
  publish_flags(flags, fl);
  if (G.prior.present != 0) publish_flags(G.prior.flags, fl_prior);
  span_end(G.stamps, t0);
  MI_TL_END(0, g, kblock);
}

// =================================================================================================
// Host side: which groups take the BCAST shape, which kernel, and their launches (bcast_site.hpp).
// =================================================================================================
static int env_int(const char* name, int fallback) {
  const char* v = std::getenv(name);
  return v != nullptr ? std::atoi(v) : fallback;
}

bool bcast_eligible(const mi_group* g) {
  if (g->num_sites != 1 || g->N < 1024 || g->K < 64) return false;
  const mi_site& st = g->sites[0];
  if (st.family > MI_BETA) return false;   // BCAST kernels exist for the first four families
  if (st.mask != nullptr && st.mask_stride_k != 0) return false;
  const mi_operand& v = g->operands[st.operand[2]];
  if (v.stride_k != 0 || v.stride_i == 0 || v.grad_mode != MI_GRAD_NONE) return false;
  for (int q = 0; q < 2; ++q) {
    const int o = st.operand[q];
    if (o < 0) continue;
    const mi_operand& op = g->operands[o];
    if (op.stride_i != 0 || op.grad_mode == MI_GRAD_DENSE) return false;
  }
  return true;
}

// Bernoulli BCAST sites over unmasked contiguous data run k_site_bcast_smem.
bool bcast_smem(const mi_group* g) {
  const mi_site& st = g->sites[0];
  return (st.family == MI_BERNOULLI_LOGITS || st.family == MI_BERNOULLI_PROBS) &&
         st.mask == nullptr && g->operands[st.operand[2]].stride_i == 1;
}

// Chunks of at most 4096 elements (measured r02: 4096 against 2048 / 8192), sized so that chunks x
// particle blocks come close to kSmemSlots workgroups: four 4-wave workgroups per CU on 256 CUs, one
// round. (r05 used 4096-element chunks throughout: C2's 245 chunks x 4 particle blocks left 44 of
// the 1024 slots idle; r06: 1280 / 1536 slots at 78 VGPR measured slower, ab14.)
constexpr int64_t kSmemSlots = 1024;

// Grids of 4096-element chunks between half a round and one round of slots are evened out to one
// round; smaller grids keep 4096 (shorter chunks would only add partials for the reduction).
int smem_chunk(int64_t N, int64_t gy) {
  gy = std::max<int64_t>(1, gy);
  const int64_t blocks = ceil_div(N, mi::kSmemMaxChunk) * gy;
  if (blocks < kSmemSlots / 2 || blocks > kSmemSlots) return mi::kSmemMaxChunk;
  const int64_t chunk = (ceil_div(N, kSmemSlots / gy) + 31) / 32 * 32;
  return (int)std::min<int64_t>(mi::kSmemMaxChunk, std::max<int64_t>(2048, chunk));
}

// The slot value of a k_site_bcast_smem launch in the rank-one layout (mi_reduce.rank1): one
// slot, and a segment list short enough for the one-launch finalize / the fused reduction.
bool smem_rank1(const mi_group* g, int64_t nseg) {
  return g->num_slots == 1 && g->compute_grads && nseg >= 3 && nseg <= MI_REDUCE_MAX_SEG;
}

namespace {

// The workgroups of the matrix instantiation with CPW chunks each that the current device holds at
// once: compute units x the runtime's occupancy answer for that instantiation (registers and LDS),
// asked once per instantiation and device. 0: the runtime gave no answer.
template <int FAM, int CPW>
int64_t smem_matrix_slots() {
  constexpr int kDevices = 16;
  static std::atomic<int64_t> cache[kDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const bool keep = dev >= 0 && dev < kDevices;
  if (keep) {
    const int64_t v = cache[dev].load(std::memory_order_relaxed);
    if (v != 0) return v;
  }
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, mi::k_site_bcast_smem<FAM, kSmemP, false, true, CPW>, mi::kBcastThreads, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const int64_t v = (int64_t)per_cu * (int64_t)cus;
  if (keep) cache[dev].store(v, std::memory_order_relaxed);
  return v;
}

// Chunks per workgroup of a matrix launch: the smallest of {1, 2, 4} whose grid, chunk groups x
// particle blocks, fits one round of resident workgroups, else 4. A grid that fits as it is keeps
// 1: the launch it always was. C2 (255 chunks x 4 particle blocks, two workgroups on each of 256
// CUs): 2, 128 groups x 4 = 512 workgroups. MININF_AMD_BCAST_CPW = 1, 2 or 4 forces it (0, unset:
// this choice).
template <int FAM>
int smem_cpw(int64_t chunks, int64_t gy) {
  const int forced = env_int("MININF_AMD_BCAST_CPW", 0);
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  const int64_t one = smem_matrix_slots<FAM, 1>();
  if (one <= 0 || chunks * gy <= one) return 1;
  const int64_t two = smem_matrix_slots<FAM, 2>();
  if (two <= 0) return 1;
  return ceil_div(chunks, 2) * gy <= two ? 2 : 4;
}

template <int FAM>
void launch_smem(const mi_group& G, int64_t nseg, dim3 plan_grid, int chunk, float* part,
                 uint32_t* flags, hipStream_t s, double* ksum) {
  const dim3 block(mi::kBcastThreads);
  // plan_grid = (chunks + side blocks, particle blocks): the kernel takes them as one XCD-aware
  // dimension (see k_site_bcast_smem)
  const int64_t chunks = nseg - 1;
  const int64_t side = (int64_t)plan_grid.x - chunks;
  const int gy = (int)plan_grid.y;
  const dim3 grid((unsigned)(ceil_div(chunks, 8) * 8 * gy + side));
  // bit 1: progress-balanced priorities; bit 2: particle-summed values
  const int rank1 = (smem_rank1(&G, nseg) ? 1 : 0) | 2 | (ksum != nullptr ? 4 : 0);
  // MININF_AMD_BCAST_SUFFSTAT=1: the reducible-floor measurement of bench.py (sum_i x_i l_k as
  // l_k sum_i x_i), never the default
  if (env_int("MININF_AMD_BCAST_SUFFSTAT", 0) != 0)
    hipLaunchKernelGGL((mi::k_site_bcast_smem<FAM, kSmemP, true>), grid, block, 0, s,
                       G, part, nseg, gy, rank1, chunk, flags, ksum);
  // MININF_AMD_BCAST_MFMA (default on): the instantiation whose chunks of 0/1 data take the matrix
  // loop; 0 launches the scalar-load kernel as it was.
  // No size or alignment threshold: the chunk reaches the matrix cores through LDS, staged by the
  // chunk-sum pass at any alignment and length, and no shape measured ran slower than the
  // scalar-load kernel (us per launch with its finalize, replayed, matrix / scalar-load kernel:
  // K 4096 n 1e6 36.6 / 74.2, the same with x one element off 16-byte alignment 41.5 / 75.3,
  // K 64 n 1e6 17.0 / 33.4, K 256 n 1e6 17.5 / 33.9, K 64 n 1024 13.9 / 16.8, K 4096 n 4096
  // 22.0 / 35.0, K 1024 n 65536 19.8 / 32.8; uniform random x, every chunk falling back to the
  // scalar-load loop at two waves per SIMD, 98.7 / 96.7).
  // (Those figures are the one-chunk launch's. Re-measured with several chunks per workgroup in
  // the tree, parent / this kernel: K 4096 n 1e6 36.6 / 33.5 at two chunks per workgroup, one
  // element off alignment 41.4 / 38.9, uniform random x 99.6 / 92.5; the shapes that keep one chunk
  // 0.3-0.5 us slower, K 64 n 1e6 16.9 / 17.2, K 256 n 1e6 17.5 / 17.8, K 64 n 1024 14.0 / 14.4,
  // K 4096 n 4096 22.1 / 22.5, K 1024 n 65536 19.7 / 20.2: DESIGN.md section 0q.)
  // (With the int8 loop, bf16 loop / int8 loop: K 4096 n 1e6 33.3 / 27.3, one element off alignment
  // 38.9 / 32.8, K 64 n 1e6 17.2 / 16.0, K 256 n 1e6 17.9 / 16.6, K 64 n 1024 14.3 / 13.6, K 4096
  // n 4096 22.5 / 20.1, K 1024 n 65536 20.2 / 17.8, uniform random x 92.3 / 92.1: section 0r.)
  // Chunks per workgroup (above): 1 launches the grid above; 2 and 4 launch one workgroup per
  // (chunk group, particle block) behind the side job's workgroups, those padded to a multiple of 8.
  else if (env_int("MININF_AMD_BCAST_MFMA", 1) != 0) {
    const int cpw = smem_cpw<FAM>(chunks, gy);
    const dim3 grouped((unsigned)(ceil_div(ceil_div(chunks, cpw), 8) * 8 * gy + ceil_div(side, 8) * 8));
    if (cpw == 4)
      hipLaunchKernelGGL((mi::k_site_bcast_smem<FAM, kSmemP, false, true, 4>), grouped, block, 0, s,
                         G, part, nseg, gy, rank1, chunk, flags, ksum);
    else if (cpw == 2)
      hipLaunchKernelGGL((mi::k_site_bcast_smem<FAM, kSmemP, false, true, 2>), grouped, block, 0, s,
                         G, part, nseg, gy, rank1, chunk, flags, ksum);
    else
      hipLaunchKernelGGL((mi::k_site_bcast_smem<FAM, kSmemP, false, true>), grid, block, 0, s, G,
                         part, nseg, gy, rank1, chunk, flags, ksum);
  } else
    hipLaunchKernelGGL((mi::k_site_bcast_smem<FAM, kSmemP>), grid, block, 0, s, G,
                       part, nseg, gy, rank1, chunk, flags, ksum);
}

template <int FAM>
int launch_prep_site(const mi_group& G, float* prep, float* part, int64_t nseg, dim3 grid,
                     uint32_t* flags, void* start_event, hipStream_t s) {
  hipLaunchKernelGGL((mi::k_bcast_prep<FAM>), dim3((unsigned)ceil_div(G.K, 256)), dim3(256), 0, s,
                     G, prep, flags);
  if (start_event != nullptr) {
    const hipError_t e = mi_record_event(start_event, s);
    if (e != hipSuccess) return to_code(e);
  }
  if (G.sites[0].mask != nullptr)
    hipLaunchKernelGGL((mi::k_site_bcast<FAM, true>), grid, dim3(mi::kBcastThreads), 0, s, G, prep,
                       part, nseg, flags);
  else
    hipLaunchKernelGGL((mi::k_site_bcast<FAM, false>), grid, dim3(mi::kBcastThreads), 0, s, G, prep,
                       part, nseg, flags);
  return 0;
}

}  // namespace

int bcast_launch(const mi_group& G, float* prep, float* part, int64_t nseg, dim3 grid,
                 uint32_t* flags, void* start_event, hipStream_t stream) {
  switch (G.sites[0].family) {
#define MI_LAUNCH_BCAST(FAM) \
  case FAM: return launch_prep_site<FAM>(G, prep, part, nseg, grid, flags, start_event, stream);
    MI_LAUNCH_BCAST(MI_BERNOULLI_LOGITS)
    MI_LAUNCH_BCAST(MI_BERNOULLI_PROBS)
    MI_LAUNCH_BCAST(MI_NORMAL)
    MI_LAUNCH_BCAST(MI_BETA)
#undef MI_LAUNCH_BCAST
    default: return MI_EUNSUPPORTED;
  }
}

void bcast_launch_smem(const mi_group& G, float* part, int64_t nseg, dim3 grid, int chunk,
                       uint32_t* flags, double* ksum, hipStream_t stream) {
  if (G.sites[0].family == MI_BERNOULLI_PROBS)
    launch_smem<MI_BERNOULLI_PROBS>(G, nseg, grid, chunk, part, flags, stream, ksum);
  else
    launch_smem<MI_BERNOULLI_LOGITS>(G, nseg, grid, chunk, part, flags, stream, ksum);
}

}  // namespace mi

#ifdef MI_SITES_TIMELINE
// The timeline build's accessors (tools/c2_timeline.py): copy the rows out, clear them.
extern "C" int mi_debug_timeline(void* out, size_t bytes) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mi::g_tl), bytes, 0, hipMemcpyDeviceToHost);
}
extern "C" int mi_debug_timeline_clear() {
  void* rows = nullptr;
  hipError_t e = hipGetSymbolAddress(&rows, HIP_SYMBOL(mi::g_tl));
  if (e == hipSuccess) e = hipMemset(rows, 0, sizeof(unsigned long long) * mi::kTimelineRows * 8);
  return (int)e;
}
#endif
