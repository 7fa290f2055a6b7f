// Posterior-predictive draws of the discrete and heavy-tailed site families.
//
// Replaces `distribution.sample(sample_shape)` (reference core.py:192-204, SampleTracer.sample) for
// the sites broadcast_samples has to simulate: Bernoulli, Exponential, Laplace, Cauchy, HalfCauchy,
// HalfNormal, LogNormal (mi_predictive_sample), Categorical (mi_predictive_categorical), the
// marginalised Normal mixture (mi_predictive_mixture_normal) and Poisson (mi_predictive_poisson), on
// the counter-based Philox generator of the guide draws.
//
// Layout: the logical space is [S, M] (S samples, M elements per sample), flat element
// e = s * M + j, the layout mi_normal_rsample has with K = 1 and N = S * M. A parameter is a pointer
// and two element strides (stride_s, stride_j), either of which may be 0: a per-sample scalar, a
// per-element constant and a dense parameter are read where they lie. A value is a function of
// (seed, stream_id, s, j, M) and not of S, the grid or the strides.
#include "elementwise_draw.hpp"
#include "gamma_sample.hpp"
#include "internal.hpp"

#include <algorithm>

namespace mi {

constexpr int kPredThreads = 256;
// Rows of at most this many categories belong to one thread, longer rows to one wave: up to here
// a thread's three passes over its row cost less than the wave's two reductions and its scan.
constexpr int kCategoricalThreadC = 32;

struct PredParam {
  const float* p;
  int64_t ss, sj;
};

template <int FAMILY>
__global__ __launch_bounds__(kPredThreads) void k_predictive_sample(
    const PredParam A, const PredParam B, int64_t M, int64_t N, uint64_t seed, uint32_t stream_id,
    float* __restrict__ out) {
  const int64_t quad = (int64_t)blockIdx.x * kPredThreads + threadIdx.x;
  const int64_t e0 = quad * 4;
  if (e0 >= N) return;
  constexpr bool kTwo = FAMILY == MI_PRED_LAPLACE || FAMILY == MI_PRED_CAUCHY ||
                        FAMILY == MI_PRED_LOG_NORMAL;
  float v[4];
  if (FAMILY == MI_PRED_HALF_NORMAL || FAMILY == MI_PRED_LOG_NORMAL) {
    guide_normals(seed, 0, stream_id, (uint64_t)quad, 0, v);
  } else {
    const U4 w = guide_bits(seed, 0, stream_id, 0, (uint64_t)quad, 0);
    v[0] = u01(w.x);
    v[1] = u01(w.y);
    v[2] = u01(w.z);
    v[3] = u01(w.w);
  }
  // (s, j) of the quad's first element; the other three follow by carrying j into s
  int64_t s = e0 / M, j = e0 - s * M;
  float o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    o[t] = 0.0f;
    if (e0 + t < N) {
      const float a = A.p[s * A.ss + j * A.sj];
      const float b = kTwo ? B.p[s * B.ss + j * B.sj] : 0.0f;
      o[t] = pred_draw<FAMILY>(a, b, v[t]);
      if (++j == M) {
        j = 0;
        ++s;
      }
    }
  }
  if (e0 + 4 <= N && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    *reinterpret_cast<float4*>(out + e0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (e0 + t < N) out[e0 + t] = o[t];
  }
}

// -------------------------------------------------------------------------------------------------
// Categorical: inversion of the row's cumulative weights exp(l - max l), fp32, ascending.
// -------------------------------------------------------------------------------------------------
MI_DEV float categorical_uniform(uint64_t seed, uint32_t stream_id, int64_t r) {
  const U4 w = guide_bits(seed, 0, stream_id, 0, (uint64_t)(r >> 2), 0);
  const int k = (int)(r & 3);
  return u01(k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w);
}

MI_DEV bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }

// Row r = (s * T + t) * B + b reads logits[s, b, :].
MI_DEV const float* categorical_row(const float* logits, int64_t ss, int64_t sb, int64_t T,
                                    int64_t B, int64_t r) {
  const int64_t st = r / B, b = r - st * B;
  const int64_t s = st / T;
  return logits + s * ss + b * sb;
}

// What becomes of row r's category c: the category itself ...
struct EmitCategory {
  int64_t* out;
  MI_DEV void operator()(int64_t r, int c) const { out[r] = c; }
};

// ... or the draw of that component of a Normal mixture: loc_c + scale_c * eps, eps the Box-Muller
// output r % 4 of the block of quad r / 4 on sub-stream 1 (the category's uniform is sub-stream 0).
struct EmitMixtureNormal {
  const float* loc;
  int64_t ms, mb, mc;
  const float* scale;
  int64_t ss, sb, sc;
  int64_t T, B;
  uint64_t seed;
  uint32_t stream_id;
  float* out;
  MI_DEV void operator()(int64_t r, int c) const {
    const U4 w = guide_bits(seed, 0, stream_id, 1, (uint64_t)(r >> 2), 0);
    float n0, n1;
    if ((r & 2) == 0) box_muller(w.x, w.y, n0, n1);
    else box_muller(w.z, w.w, n0, n1);
    const float eps = (r & 1) == 0 ? n0 : n1;
    out[r] = categorical_row(loc, ms, mb, T, B, r)[c * mc] +
             categorical_row(scale, ss, sb, T, B, r)[c * sc] * eps;
  }
};

template <typename Emit>
__global__ __launch_bounds__(kPredThreads) void k_categorical_thread(
    const float* __restrict__ logits, int64_t ss, int64_t sb, int64_t sc, int64_t T, int64_t B,
    int C, int64_t rows, uint64_t seed, uint32_t stream_id, const Emit emit) {
  const int64_t r = (int64_t)blockIdx.x * kPredThreads + threadIdx.x;
  if (r >= rows) return;
  const float* row = categorical_row(logits, ss, sb, T, B, r);
  const float u = categorical_uniform(seed, stream_id, r);
  float mx = -__builtin_inff();
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, row[c * sc]);
  float total = 0.0f;
  for (int c = 0; c < C; ++c) total += expf(row[c * sc] - mx);
  const float threshold = u * total;
  float cum = 0.0f;
  int found = -1, last = -1;
  for (int c = 0; c < C; ++c) {
    const float l = row[c * sc];
    cum += expf(l - mx);
    if (found < 0 && cum > threshold) found = c;
    if (finite_f(l)) last = c;
  }
  emit(r, found >= 0 ? found : (last >= 0 ? last : C - 1));
}

template <typename Emit>
__global__ __launch_bounds__(kPredThreads) void k_categorical_wave(
    const float* __restrict__ logits, int64_t ss, int64_t sb, int64_t sc, int64_t T, int64_t B,
    int C, int64_t rows, uint64_t seed, uint32_t stream_id, const Emit emit) {
  constexpr int kWaves = kPredThreads / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t first = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  // lane i owns the contiguous categories [i * chunk, (i + 1) * chunk)
  const int chunk = (C + kWave - 1) / kWave;
  const int c0 = min(C, lane * chunk), c1 = min(C, c0 + chunk);
  for (int64_t r = first; r < rows; r += stride) {
    const float* row = categorical_row(logits, ss, sb, T, B, r);
    const float u = categorical_uniform(seed, stream_id, r);
    float mx = -__builtin_inff();
    int last = -1;
    for (int c = c0; c < c1; ++c) {
      const float l = row[c * sc];
      mx = fmaxf(mx, l);
      if (finite_f(l)) last = c;
    }
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, offset, kWave));
      last = max(last, __shfl_xor(last, offset, kWave));
    }
    float local = 0.0f;
    for (int c = c0; c < c1; ++c) local += expf(row[c * sc] - mx);
    // inclusive prefix sum of the lanes' chunk sums
    float incl = local;
#pragma unroll
    for (int offset = 1; offset < kWave; offset <<= 1) {
      const float below = __shfl_up(incl, offset, kWave);
      if (lane >= offset) incl += below;
    }
    const float total = __shfl(incl, kWave - 1, kWave);
    float cum = __shfl_up(incl, 1, kWave);
    if (lane == 0) cum = 0.0f;
    const float threshold = u * total;
    int found = C;
    for (int c = c0; c < c1; ++c) {
      cum += expf(row[c * sc] - mx);
      if (found == C && cum > threshold) found = c;
    }
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1)
      found = min(found, __shfl_xor(found, offset, kWave));
    if (lane == 0) emit(r, found < C ? found : (last >= 0 ? last : C - 1));
  }
}

// -------------------------------------------------------------------------------------------------
// Poisson on the element-keyed stream (gamma_sample.hpp Stream, sub-stream 3).
// rate < 10: Knuth's product of uniforms, fp32. rate >= 10: the transformed rejection PTRS of
// W. Hoermann, "The transformed rejection method for generating Poisson random variables",
// Insurance: Mathematics and Economics 12 (1993), 39-45, in fp64: at rate 1e6 the three terms of
// its log acceptance bound are near 1.4e7, where an fp32 lgammaf resolves 1 while the bound decides
// within a few tenths (the sum's own size); fp64 keeps the decision that of the formula.
// Every loop is bounded: at most 250 factors (P(Poisson(10) > 250) < 1e-200) and 64 attempts of
// two uniforms (acceptance > 0.86 per attempt), so a draw reads at most 64 blocks of its stream
// and no input can spin a wave.
// -------------------------------------------------------------------------------------------------
constexpr int kPoissonFactors = 250;
constexpr int kPoissonAttempts = 64;

MI_DEV float sample_poisson(float rate, Stream& rng) {
  if (!(rate >= 0.0f) || !finite_f(rate)) return __builtin_nanf("");
  if (rate == 0.0f) return 0.0f;
  if (rate < 10.0f) {
    const float limit = expf(-rate);
    float p = rng.uniform();
    int k = 0;
    while (p >= limit && k < kPoissonFactors) {
      ++k;
      p *= rng.uniform();
    }
    return (float)k;
  }
  const double lam = (double)rate;
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int attempt = 0; attempt < kPoissonAttempts; ++attempt) {
    const double U = (double)rng.uniform() - 0.5;
    const double V = (double)rng.uniform();
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return (float)k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0))
      return (float)k;
  }
  return (float)floor(lam);   // not reached in practice
}

__global__ __launch_bounds__(kPredThreads) void k_predictive_poisson(
    const PredParam R, int64_t M, int64_t N, uint64_t seed, uint32_t stream_id,
    float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kPredThreads + threadIdx.x;
  if (e >= N) return;
  const int64_t s = e / M, j = e - s * M;
  Stream rng{seed, 0, stream_id, 3u, (uint64_t)e, 0};
  out[e] = sample_poisson(R.p[s * R.ss + j * R.sj], rng);
}

template <int FAMILY>
static void launch_sample(const PredParam& A, const PredParam& B, int64_t M, int64_t N,
                          uint64_t seed, uint32_t stream_id, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_predictive_sample<FAMILY>,
                     dim3((unsigned)ceil_div(N, 4 * (int64_t)kPredThreads)), dim3(kPredThreads), 0,
                     stream, A, B, M, N, seed, stream_id, out);
}

}  // namespace mi

namespace {

constexpr int64_t kMaxQuadElements = (int64_t)1 << 34;   // 32-bit quad counter
constexpr int64_t kMaxStreamElements = (int64_t)1 << 32; // 32-bit element counter

// S * M without overflow: -1 when it exceeds `cap`.
int64_t bounded_product(int64_t S, int64_t M, int64_t cap) {
  if (S > cap / M) return -1;
  const int64_t n = S * M;
  return n <= cap ? n : -1;
}

// The category of each of the S * T * B rows, handed to `emit` (the argument checks and the two
// kernels of mi_predictive_categorical).
template <typename Emit>
int launch_categorical(const float* logits, int64_t stride_s, int64_t stride_b, int64_t stride_c,
                       int64_t S, int64_t T, int64_t B, int64_t C, uint64_t seed,
                       uint32_t stream_id, const Emit& emit, void* stream) {
  if (logits == nullptr || S < 1 || T < 1 || B < 1 || C < 1 || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  if (C > MI_PRED_CATEGORICAL_MAX_C) return MI_EUNSUPPORTED;
  const int64_t ST = bounded_product(S, T, kMaxQuadElements);
  const int64_t rows = ST < 0 ? -1 : bounded_product(ST, B, kMaxQuadElements);
  if (rows < 0) return MI_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C <= mi::kCategoricalThreadC) {
    hipLaunchKernelGGL(mi::k_categorical_thread<Emit>,
                       dim3((unsigned)ceil_div(rows, (int64_t)mi::kPredThreads)),
                       dim3(mi::kPredThreads), 0, s, logits, stride_s, stride_b, stride_c, T, B,
                       (int)C, rows, seed, stream_id, emit);
  } else {
    // one wave per row, the waves striding over the rows when there are more than the grid holds
    const int64_t blocks = std::min<int64_t>(ceil_div(rows, mi::kPredThreads / mi::kWave), 1 << 20);
    hipLaunchKernelGGL(mi::k_categorical_wave<Emit>, dim3((unsigned)blocks),
                       dim3(mi::kPredThreads), 0, s, logits, stride_s, stride_b, stride_c, T, B,
                       (int)C, rows, seed, stream_id, emit);
  }
  return to_code(hipGetLastError());
}

}  // namespace

extern "C" {

int mi_predictive_sample(int family, const float* a, int64_t a_stride_s, int64_t a_stride_j,
                         const float* b, int64_t b_stride_s, int64_t b_stride_j, int64_t S,
                         int64_t M, uint64_t seed, uint32_t stream_id, float* out, void* stream) {
  if (family < 0 || family >= MI_PRED_FAMILIES || a == nullptr || out == nullptr || S < 1 ||
      M < 1 || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  const bool two = family == MI_PRED_LAPLACE || family == MI_PRED_CAUCHY ||
                   family == MI_PRED_LOG_NORMAL;
  if (two && b == nullptr) return MI_EINVAL;
  const int64_t N = bounded_product(S, M, kMaxQuadElements);
  if (N < 0) return MI_EUNSUPPORTED;
  const mi::PredParam A{a, a_stride_s, a_stride_j};
  const mi::PredParam B{two ? b : a, two ? b_stride_s : 0, two ? b_stride_j : 0};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (family) {
    case MI_PRED_BERNOULLI_PROBS:
      mi::launch_sample<MI_PRED_BERNOULLI_PROBS>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_BERNOULLI_LOGITS:
      mi::launch_sample<MI_PRED_BERNOULLI_LOGITS>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_EXPONENTIAL:
      mi::launch_sample<MI_PRED_EXPONENTIAL>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_LAPLACE:
      mi::launch_sample<MI_PRED_LAPLACE>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_CAUCHY:
      mi::launch_sample<MI_PRED_CAUCHY>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_HALF_CAUCHY:
      mi::launch_sample<MI_PRED_HALF_CAUCHY>(A, B, M, N, seed, stream_id, out, s);
      break;
    case MI_PRED_HALF_NORMAL:
      mi::launch_sample<MI_PRED_HALF_NORMAL>(A, B, M, N, seed, stream_id, out, s);
      break;
    default:
      mi::launch_sample<MI_PRED_LOG_NORMAL>(A, B, M, N, seed, stream_id, out, s);
      break;
  }
  return to_code(hipGetLastError());
}

int mi_predictive_categorical(const float* logits, int64_t stride_s, int64_t stride_b,
                              int64_t stride_c, int64_t S, int64_t T, int64_t B, int64_t C,
                              uint64_t seed, uint32_t stream_id, int64_t* out, void* stream) {
  if (out == nullptr) return MI_EINVAL;
  return launch_categorical(logits, stride_s, stride_b, stride_c, S, T, B, C, seed, stream_id,
                            mi::EmitCategory{out}, stream);
}

int mi_predictive_mixture_normal(const float* logits, int64_t logits_stride_s,
                                 int64_t logits_stride_b, int64_t logits_stride_c,
                                 const float* loc, int64_t loc_stride_s, int64_t loc_stride_b,
                                 int64_t loc_stride_c, const float* scale, int64_t scale_stride_s,
                                 int64_t scale_stride_b, int64_t scale_stride_c, int64_t S,
                                 int64_t T, int64_t B, int64_t C, uint64_t seed,
                                 uint32_t stream_id, float* out, void* stream) {
  if (loc == nullptr || scale == nullptr || out == nullptr) return MI_EINVAL;
  const mi::EmitMixtureNormal emit{loc,  loc_stride_s, loc_stride_b, loc_stride_c,
                                   scale, scale_stride_s, scale_stride_b, scale_stride_c,
                                   T,    B,            seed,         stream_id,
                                   out};
  return launch_categorical(logits, logits_stride_s, logits_stride_b, logits_stride_c, S, T, B, C,
                            seed, stream_id, emit, stream);
}

int mi_predictive_poisson(const float* rate, int64_t stride_s, int64_t stride_j, int64_t S,
                          int64_t M, uint64_t seed, uint32_t stream_id, float* out, void* stream) {
  if (rate == nullptr || out == nullptr || S < 1 || M < 1 || stream_id > 0xFFFFFFu)
    return MI_EINVAL;
  const int64_t N = bounded_product(S, M, kMaxStreamElements);
  if (N < 0) return MI_EUNSUPPORTED;
  const mi::PredParam R{rate, stride_s, stride_j};
  hipLaunchKernelGGL(mi::k_predictive_poisson,
                     dim3((unsigned)ceil_div(N, (int64_t)mi::kPredThreads)),
                     dim3(mi::kPredThreads), 0, static_cast<hipStream_t>(stream), R, M, N, seed,
                     stream_id, out);
  return to_code(hipGetLastError());
}

}  // extern "C"
