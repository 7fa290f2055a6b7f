// Softmax regression sites: Categorical(logits = X @ Theta) with Theta [K, P, C], the product
// evaluated inside the site kernel (include/mininf_amd.h, mi_softmax_linear).
//
// Traced over K particles the model's `X @ Theta` is a [K, N, C] GEMM whose output is read once by
// mi_categorical_forward, which writes a [K, N, C] gradient that a second GEMM reduces. Here, per
// 32-row tile of X, 32 particles and category c, with the tile toolkit's layouts (mfma_tile.hpp)
// and the two-product scheme of linear.hip:
//   MU_c[i, k]    = sum_p X[i, p] Theta[k, p, c]            (v_mfma_f32_32x32x2_f32, A = X, B = Theta_c^T)
//   m, s          = max_c MU_c, sum_c exp(MU_c - m)         (VALU, running over c, per (i, k))
//   R_c[i, k]     = mask_i ([c == y_i] - exp(MU_c - m) / s) (VALU, in the accumulator registers)
//   DTH_c[k, p]  += sum_i R_c[i, k] X[i, p]                 (v_mfma_f32_32x32x2_f32, A = R_c^T, B = X)
// The accumulator of the first product is already the A operand of the second (linear.hip's
// header), so neither the logits nor their gradient leave the registers.
//
// Split: a block takes 32 particles and stages of 256 / PT rows (PT = 1 or 2 feature tiles of 32),
// X staged once per stage in LDS; wave w owns the stage's row tiles w * TPW .. w * TPW + TPW - 1.
// The register file cannot hold MU_c or DTH_c for all C categories, so a stage runs the
// categories twice. Pass 1: for every c the wave's MU_c tiles update (m, s) in registers (64 of
// them at most), and eta_y - m - log s joins the value in fp64. Pass 2: for every c the first
// product is repeated (the same instructions in the same order: bit-identical MU_c, so
// MU_c - m <= 0 holds exactly), turned into R_c and contracted with X into one DTH_c accumulator,
// whose four waves' tiles are summed through LDS in a fixed order (fp64) and added to the block's
// partial tile. The price is 3 rather than 2 products per category; in return the kernel has one
// instantiation per PT, whatever C, and small register and LDS budgets (two blocks per CU).
// Per-(row block, particle) partials are reduced in fp64 in a fixed order by k_softmax_finish:
// no floating-point atomics.
#include "common.hpp"
#include "internal.hpp"
#include "mfma_tile.hpp"

namespace mi {

constexpr int kSmThreads = 256;
constexpr int kSmWaves = kSmThreads / kWave;

template <int PT>
struct SmShape {
  static constexpr int PM = 32 * PT;            // padded features
  static constexpr int HS = 16 * PT;            // floats per feature-parity half of an LDS row
  static constexpr int RSTR = PM + 4;           // LDS row stride (floats), as k_linear_mfma's
  static constexpr int ROWS = 256 / PT;         // rows per stage
  static constexpr int TPW = ROWS / 32 / kSmWaves;   // 32-row tiles per wave and stage
};

__device__ __forceinline__ bool sm_non_finite(float x) { return !(fabsf(x) < __builtin_inff()); }

// Grid: gx * gy blocks; block b takes particle tile b % gy and row block b / gy (stages
// [rb * spb, (rb + 1) * spb)). part: [gx][K][C][P] floats; tpart: [gx][K] doubles.
template <int PT>
__global__ __launch_bounds__(kSmThreads, 2) void k_softmax_linear(const mi_softmax_linear L, int gy,
                                                                  int64_t spb,
                                                                  float* __restrict__ part,
                                                                  double* __restrict__ tpart,
                                                                  uint32_t* __restrict__ flags,
                                                                  int grads) {
  using S = SmShape<PT>;
  __shared__ __attribute__((aligned(16))) float xs[S::ROWS * S::RSTR];
  __shared__ int labs[S::ROWS];      // the row's label, -1 where no category matches (or masked)
  __shared__ int obsv[S::ROWS];      // 1: an observed row of the data
  __shared__ float red[kSmWaves * 16 * kWave];
  __shared__ double tred[kSmWaves * 32];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int h = lane >> 5, c = lane & 31;
  const int64_t K = L.K, N = L.N;
  const int P = (int)L.P, C = (int)L.C;
  const int64_t rb = (int64_t)blockIdx.x / gy;
  const int64_t k0 = ((int64_t)blockIdx.x % gy) * 32;
  const int64_t kk = k0 + c;
  const bool kin = kk < K;
  const float* const thp = L.theta + (kin ? kk : K - 1) * L.theta_stride_k;
  uint32_t fl = 0u;
  double lpd = 0.0;   // sum over this lane's (row, particle k0 + c) of eta_y - m - log s

  // B fragment of the first product for category cat: Theta[k0 + c][2 s + h][cat], every load
  // from a clamped (valid) address and zeroed after.
  auto load_theta = [&](int cat, float (&thf)[S::HS]) {
#pragma unroll
    for (int s = 0; s < S::HS; ++s) {
      const int p = 2 * s + h;
      const float v = thp[(int64_t)(p < P ? p : P - 1) * L.theta_stride_j + (int64_t)cat * L.theta_stride_c];
      thf[s] = keep_if(v, kin && p < P);
    }
  };
  // MU_cat of the tile's 32 rows and the block's 32 particles
  auto gemm1 = [&](int tile, const float (&thf)[S::HS]) -> f32x16 {
    f32x16 mu = f32x16{};
    const float* xa = xs + (tile * 32 + c) * S::RSTR + h * S::HS;
#pragma unroll
    for (int s = 0; s < S::HS; s += 4) {
      const float4 a = *reinterpret_cast<const float4*>(xa + s);
      mu = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, thf[s + 0], mu, 0, 0, 0);
      mu = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, thf[s + 1], mu, 0, 0, 0);
      mu = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, thf[s + 2], mu, 0, 0, 0);
      mu = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, thf[s + 3], mu, 0, 0, 0);
    }
    return mu;
  };

  const int64_t nstage = (N + S::ROWS - 1) / S::ROWS;
  const int64_t st0 = rb * spb;
  const int64_t st1 = min(nstage, st0 + spb);
  for (int64_t st = st0; st < st1; ++st) {
    const int64_t row0 = st * S::ROWS;
    __syncthreads();   // the previous stage's readers of xs / labs / obsv are done
    // ---- staging: X as [row][feature parity][feature / 2], zero past N and P ------------------
    for (int e = tid; e < S::ROWS * S::PM; e += kSmThreads) {
      const int rr = e / S::PM, p = e % S::PM;
      const int64_t row = row0 + rr;
      float v = 0.0f;
      if (row < N && p < P) {
        const int64_t i = L.row_index != nullptr ? (int64_t)L.row_index[row] : row;
        v = L.x[i * L.x_stride_i + (int64_t)p * L.x_stride_j];
      }
      xs[rr * S::RSTR + (p & 1) * S::HS + (p >> 1)] = v;
    }
    for (int rr = tid; rr < S::ROWS; rr += kSmThreads) {
      const int64_t row = row0 + rr;
      int lab = -1, ob = 0;
      if (row < N) {
        const int64_t i = L.row_index != nullptr ? (int64_t)L.row_index[row] : row;
        ob = (L.mask == nullptr || L.mask[i * L.mask_stride_i] != 0) ? 1 : 0;
        if (ob) {   // (a masked-out row's label is never looked at)
          bool ok;
          int64_t y;
          if (L.value_kind == MI_SOFTMAX_LABEL_FLOAT32) {
            const float yf = static_cast<const float*>(L.value)[i * L.value_stride_i];
            ok = yf >= 0.0f && yf < (float)C && yf == floorf(yf);   // (false for NaN)
            y = ok ? (int64_t)yf : -1;
          } else {
            y = static_cast<const int64_t*>(L.value)[i * L.value_stride_i];
            ok = y >= 0 && y < C;
          }
          lab = ok ? (int)y : -1;
          fl |= ok ? 0u : MI_FLAG_SUPPORT;
        }
      }
      labs[rr] = lab;
      obsv[rr] = ob;
    }
    __syncthreads();

    // ---- pass 1: running (max, sum of exp) over the categories, and the value -----------------
    float m[S::TPW][16], sm[S::TPW][16];
#pragma unroll
    for (int j = 0; j < S::TPW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        m[j][r] = -__builtin_inff();
        sm[j][r] = 0.0f;
      }
#pragma unroll 1
    for (int cat = 0; cat < C; ++cat) {
      float thf[S::HS];
      load_theta(cat, thf);
#pragma unroll
      for (int j = 0; j < S::TPW; ++j) {
        const int tile = wave * S::TPW + j;
        const f32x16 mu = gemm1(tile, thf);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = tile * 32 + acc_row(r, lane);
          const float e = mu[r];
          fl |= (obsv[row] != 0 && sm_non_finite(e)) ? MI_FLAG_PARAM : 0u;
          const float mn = fmaxf(m[j][r], e);
          sm[j][r] = fmaf(sm[j][r], fast_exp(m[j][r] - mn), fast_exp(e - mn));
          m[j][r] = mn;
          if (labs[row] == cat) lpd += (double)e;
        }
      }
    }
    // 1 / s replaces s; the value loses m + log s on observed rows
#pragma unroll
    for (int j = 0; j < S::TPW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (wave * S::TPW + j) * 32 + acc_row(r, lane);
        const float ls = __builtin_amdgcn_logf(sm[j][r]) * 0.69314718055994531f;
        if (obsv[row] != 0) lpd -= (double)m[j][r] + (double)ls;
        sm[j][r] = rcp(sm[j][r]);
      }

    // ---- pass 2: R_c and DTH_c, category by category -----------------------------------------
    if (grads) {
#pragma unroll 1
      for (int cat = 0; cat < C; ++cat) {
        float thf[S::HS];
        load_theta(cat, thf);
        f32x16 acc2[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) acc2[t] = f32x16{};
#pragma unroll
        for (int j = 0; j < S::TPW; ++j) {
          const int tile = wave * S::TPW + j;
          f32x16 mu = gemm1(tile, thf);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = tile * 32 + acc_row(r, lane);
            const float pc = fast_exp(mu[r] - m[j][r]) * sm[j][r];
            const float d = (labs[row] == cat ? 1.0f : 0.0f) - pc;
            mu[r] = obsv[row] != 0 ? d : 0.0f;
          }
          // DTH[k, p] += sum_rows R[row, k] X[row, p]: k-step r pairs register r with its row
#pragma unroll
          for (int t = 0; t < PT; ++t) {
            const int p = 32 * t + c;
            const float* xb = xs + (p & 1) * S::HS + (p >> 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = tile * 32 + acc_row(r, lane);
              acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(mu[r], xb[row * S::RSTR], acc2[t], 0, 0, 0);
            }
          }
        }
        // the four waves' tiles of each feature tile, summed in wave order; wave w sums and
        // writes registers [4 w, 4 w + 4) of every lane
#pragma unroll
        for (int t = 0; t < PT; ++t) {
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * kWave + lane] = acc2[t][r];
          __syncthreads();
#pragma unroll
          for (int q = 0; q < 16 / kSmWaves; ++q) {
            const int r = wave * (16 / kSmWaves) + q;
            double d = 0.0;
#pragma unroll
            for (int w = 0; w < kSmWaves; ++w) d += (double)red[(w * 16 + r) * kWave + lane];
            const int64_t kq = k0 + acc_row(r, lane);
            const int p = 32 * t + c;
            if (kq < K && p < P) {
              float* dst = part + ((rb * K + kq) * C + cat) * P + p;
              *dst = st == st0 ? (float)d : (float)((double)*dst + d);
            }
          }
          __syncthreads();
        }
      }
    }
  }

  // ---- the value: the lane halves, then the four waves in wave order --------------------------
  lpd += __shfl_xor(lpd, 32, kWave);
  if (h == 0) tred[wave * 32 + c] = lpd;
  __syncthreads();
  if (wave == 0 && h == 0 && kin) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kSmWaves; ++w) v += tred[w * 32 + c];
    tpart[rb * K + kk] = v;
  }
  publish_flags(flags, fl);
}

// total[k] = scale * sum_tiles tpart; dtheta[k][p][c] = gscale * sum_tiles part[tile][k][c][p]
// (tiles ascending, fp64).
__global__ __launch_bounds__(256) void k_softmax_finish(const float* __restrict__ part,
                                                        const double* __restrict__ tpart,
                                                        int64_t ntile, int64_t K, int64_t P, int64_t C,
                                                        double scale, double gscale,
                                                        float* __restrict__ total,
                                                        float* __restrict__ dtheta) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t slots = K * C * P;
  if (idx < K) {
    double v = 0.0;
    for (int64_t t = 0; t < ntile; ++t) v += tpart[t * K + idx];
    total[idx] = (float)(scale * v);
    return;
  }
  const int64_t j = idx - K;
  if (dtheta == nullptr || j >= slots) return;
  double v = 0.0;
  for (int64_t t = 0; t < ntile; ++t) v += (double)part[t * slots + j];
  const int64_t k = j / (C * P), cat = (j / P) % C, p = j % P;
  dtheta[(k * P + p) * C + cat] = (float)(gscale * v);
}

}  // namespace mi

namespace {

bool valid(const mi_softmax_linear* L) {
  return L != nullptr && L->K >= 1 && L->N >= 1 && L->P >= 1 && L->P <= MI_LINEAR_MAX_P &&
         L->C >= 1 && L->C <= MI_SOFTMAX_LINEAR_MAX_C && L->x != nullptr && L->theta != nullptr &&
         L->value != nullptr &&
         (L->value_kind == MI_SOFTMAX_LABEL_INT64 || L->value_kind == MI_SOFTMAX_LABEL_FLOAT32);
}

struct Geometry {
  int pt;
  int64_t gx, gy, spb;
};

Geometry geometry(const mi_softmax_linear* L) {
  Geometry g{};
  g.pt = L->P <= 32 ? 1 : 2;
  g.gy = ceil_div(L->K, 32);
  const int64_t nstage = ceil_div(L->N, 256 / g.pt);
  // about 1024 blocks over the grid, whole stages per block
  const int64_t target = std::max<int64_t>(1, 1024 / g.gy);
  g.spb = ceil_div(nstage, target);
  g.gx = ceil_div(nstage, g.spb);
  return g;
}

size_t part_bytes(const mi_softmax_linear* L, const Geometry& g) {
  return ((size_t)g.gx * (size_t)L->K * (size_t)L->C * (size_t)L->P * sizeof(float) + 255) / 256 * 256;
}

}  // namespace

extern "C" {

int mi_softmax_linear_struct_size(size_t* bytes) {
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = sizeof(mi_softmax_linear);
  return 0;
}

int mi_softmax_linear_workspace_bytes(const mi_softmax_linear* site, size_t* bytes) {
  if (!valid(site) || bytes == nullptr) return MI_EINVAL;
  const Geometry g = geometry(site);
  *bytes = part_bytes(site, g) + (size_t)g.gx * (size_t)site->K * sizeof(double);
  return 0;
}

int mi_softmax_linear_forward(const mi_softmax_linear* site, void* workspace, size_t workspace_bytes,
                              float* total, float* dtheta, uint32_t* flags, void* stream) {
  if (!valid(site) || total == nullptr || flags == nullptr) return MI_EINVAL;
  const Geometry g = geometry(site);
  if (g.gx * g.gy > kMaxGrid) return MI_EUNSUPPORTED;
  size_t need = 0;
  mi_softmax_linear_workspace_bytes(site, &need);
  if (workspace == nullptr || workspace_bytes < need) return MI_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (!(site->options & MI_GROUP_FLAGS_ZEROED)) {
    if ((e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s)) != hipSuccess) return to_code(e);
  }
  float* part = static_cast<float*>(workspace);
  double* tpart = reinterpret_cast<double*>(static_cast<char*>(workspace) + part_bytes(site, g));
  const dim3 grid((unsigned)(g.gx * g.gy));
  const int grads = dtheta != nullptr ? 1 : 0;
  if (g.pt == 1)
    hipLaunchKernelGGL((mi::k_softmax_linear<1>), grid, dim3(mi::kSmThreads), 0, s, *site, (int)g.gy,
                       g.spb, part, tpart, flags, grads);
  else
    hipLaunchKernelGGL((mi::k_softmax_linear<2>), grid, dim3(mi::kSmThreads), 0, s, *site, (int)g.gy,
                       g.spb, part, tpart, flags, grads);
  if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  const int64_t items = site->K + (grads ? site->K * site->C * site->P : 0);
  hipLaunchKernelGGL(mi::k_softmax_finish, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, s, part,
                     tpart, g.gx, site->K, site->P, site->C, site->site_scale,
                     (double)site->grad_scale * site->site_scale, total, dtheta);
  return to_code(hipGetLastError());
}

}  // extern "C"
