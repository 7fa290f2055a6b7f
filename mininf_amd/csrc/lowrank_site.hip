// Density of a LowRankMultivariateNormal site and its gradients, for K particles and N rows.
//
// Replaces LowRankMultivariateNormal.log_prob (torch 2.10 lowrank_multivariate_normal.py:203-212,
// _batch_lowrank_mahalanobis and _batch_lowrank_logdet) and the gradients autograd computes through
// the constructor's capacitance product and Cholesky, for value x[k, i, :], loc[k, :],
// W = cov_factor[k][D, R], d = cov_diag[k, :] and L = _capacitance_tril[k][R, R], the lower factor of
// C = I + W^T diag(1 / d) W. Per (k, i), with r = x_i - loc, y = r / d, t = W^T y, c = C^-1 t:
//   log_prob[k, i] = -1/2 (D log 2 pi + 2 sum_j log L[j, j] + sum_j log d[j] + r.y - t.c)
// and, for the upstream g[k, i], a_i = (r_i - W c_i) / d, G = sum_i g_i, M = W C^-1:
//   dvalue[k, i, :] = -g_i a_i                dloc[k, :] = sum_i g_i a_i
//   dcov_factor[k]  = sum_i g_i a_i c_i^T - G M / d[:, None]
//   dcov_diag[k, j] = 1/2 sum_i g_i a_ij^2 - 1/2 G (1 / d_j - (sum_r M_jr W_jr) / d_j^2)
// Forward, two launches:
//   1. a workgroup per particle, fp64 in LDS (lowrank_capacitance.hpp): B = L^-1 (handed on as f32)
//      and the log terms. C^-1 = B^T B is never formed: with R > D its product with t loses to
//      rounding what r - W c then cancels against, the two triangular factors do not;
//   2. the row pass, T = Y W, U = T B^T and coef = U B, with t.c = u.u for log_prob. R >= 32:
//      v_mfma_f32_32x32x2_f32 over the 32 x 32 tiles of mfma_tile.hpp, a wave per 32 rows and four
//      waves sharing each staged tile of W, zero-padded to whole tiles. R < 32: on the VALU, a thread
//      per row with the rank padded to 4, 8, 16 or 32 (lowrank_guide.hip says why).
// Backward, up to three launches:
//   1. launch 1 of the forward again (B, for M = (W B^T) B), when dcov_factor or dcov_diag is asked
//      for;
//   2. a workgroup per (particle, slice of rows, 32 columns of D) on the VALU: W c_i from the staged
//      rows of W and coef, a_i, dvalue, and the slice's sums of g_i a_i, g_i a_ij^2, g_i a_i c_i^T and
//      g_i into the workspace, each a chain in row order;
//   3. a workgroup per (particle, row of W): the slices summed in order, M's row and the G terms.
// A row with g_i == 0 is not read beyond g_i: it contributes exact zeros whatever its value holds.
// Every sum has a fixed order (no atomics): two calls on the same inputs are bit-identical, and a
// gradient that is not asked for changes none of the others.
#include "internal.hpp"
#include "lowrank_capacitance.hpp"
#include "mfma_tile.hpp"

#include <algorithm>

namespace mi {

constexpr int kLsThreads = 256;     // every kernel here but the finish
constexpr int kLsChunk = 64;        // rows of W the VALU forward stages at a time
constexpr int kLsFinishThreads = 128;   // the finish: a thread per column of W (MI_LOWRANK_MAX_R)
constexpr int kLsMaxRT = MI_LOWRANK_MAX_R / kTile;
static_assert(kLsFinishThreads == MI_LOWRANK_MAX_R, "the finish has a thread per rank");

// The site's operands: every parameter through its particle stride (0: shared by the particles).
struct LsOperands {
  const float* value;
  int64_t value_sk, value_si;
  const float* loc;
  int64_t loc_sk;
  const float* W;
  int64_t W_sk;
  const float* d;
  int64_t d_sk;
  int64_t K, N, D, R;
};

// ---- B = L^-1 and the log terms, a workgroup per particle ----------------------------------------
__global__ __launch_bounds__(1024) void k_lowrank_site_capacitance(
    const float* __restrict__ L, int64_t L_sk, const float* __restrict__ d, int64_t d_sk, int R,
    int64_t D, float* __restrict__ binv, double* __restrict__ logterm) {
  extern __shared__ double X[];   // [R][R | 1], then a sum per wave
  const int64_t k = blockIdx.x;
  L += k * L_sk;
  d += k * d_sk;
  double* red = X + R * (R | 1);
  const int t = threadIdx.x, nt = blockDim.x;
  double s = 0.0;
  for (int j = t; j < R; j += nt) s += 2.0 * log((double)L[j * R + j]);
  for (int64_t j = t; j < D; j += nt) s += log((double)d[j]);
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  if ((t & (kWave - 1)) == 0) red[t >> 6] = s;
  capacitance_stage(L, R, X);
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int q = 0; q < nt / kWave; ++q) sum += red[q];
    logterm[k] = (double)D * log(2.0 * M_PI) + sum;
  }
  capacitance_factor_inverse(X, R);
  binv += k * R * R;   // B = L^-1, f32, the zeros above its diagonal included
  for (int e = t; e < R * R; e += nt) binv[e] = (float)X[(e / R) * (R | 1) + e % R];
}

// ---- the forward row pass, R < 32: a thread per row, 256 rows per workgroup ----------------------
template <int RP>
__global__ __launch_bounds__(kLsThreads) void k_lowrank_site_forward_valu(
    LsOperands a, const float* __restrict__ binv, const double* __restrict__ logterm,
    int64_t tiles, float* __restrict__ log_prob, float* __restrict__ coef) {
  __shared__ float cs[RP][RP];   // B = L^-1, zero-padded
  __shared__ float ws[kLsChunk][RP];
  __shared__ float ls[kLsChunk], is[kLsChunk];
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
  const int64_t D = a.D, R = a.R;
  const float* W = a.W + k * a.W_sk;
  const float* loc = a.loc + k * a.loc_sk;
  const float* d = a.d + k * a.d_sk;
  for (int e = t; e < RP * RP; e += kLsThreads) {
    const int s = e / RP, r = e - s * RP;
    cs[s][r] = (s < R && r < R) ? binv[(k * R + s) * R + r] : 0.0f;
  }
  const int64_t i = tile * kLsThreads + t;
  const bool active = i < a.N;
  const float* x = a.value + k * a.value_sk + (active ? i : 0) * a.value_si;
  float tt[RP];
#pragma unroll
  for (int r = 0; r < RP; ++r) tt[r] = 0.0f;
  float q = 0.0f;
  for (int64_t j0 = 0; j0 < D; j0 += kLsChunk) {
    __syncthreads();   // the previous chunk is read (and, the first time, cs is written)
    for (int e = t; e < kLsChunk * RP; e += kLsThreads) {
      const int jj = e / RP, r = e - jj * RP;
      ws[jj][r] = (j0 + jj < D && r < R) ? W[(j0 + jj) * R + r] : 0.0f;
    }
    if (t < kLsChunk) {
      const bool ok = j0 + t < D;
      ls[t] = ok ? loc[j0 + t] : 0.0f;
      is[t] = ok ? 1.0f / d[j0 + t] : 0.0f;
    }
    __syncthreads();
    if (active) {
      const int n = (int)min((int64_t)kLsChunk, D - j0);
      for (int jj = 0; jj < n; ++jj) {
        const float r = x[j0 + jj] - ls[jj];
        const float y = r * is[jj];
        q = fmaf(r, y, q);
#pragma unroll
        for (int c = 0; c < RP; ++c) tt[c] = fmaf(y, ws[jj][c], tt[c]);
      }
    }
  }
  if (!active) return;
  float u[RP], uu = 0.0f;   // u = B t, and t.c = u.u
#pragma unroll
  for (int r = 0; r < RP; ++r) {
    u[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < RP; ++s) u[r] = fmaf(cs[r][s], tt[s], u[r]);
    uu = fmaf(u[r], u[r], uu);
  }
#pragma unroll
  for (int r = 0; r < RP; ++r) {
    float c = 0.0f;   // c = B^T u
#pragma unroll
    for (int s = 0; s < RP; ++s) c = fmaf(cs[s][r], u[s], c);
    if (r < R) coef[(k * a.N + i) * R + r] = c;
  }
  log_prob[k * a.N + i] = (float)(-0.5 * (logterm[k] + ((double)q - (double)uu)));
}

// ---- the forward row pass, R >= 32: a wave per 32 rows, four waves per workgroup -----------------
// LDS: RT shared tiles -- the 32 rows of W of the step, k-major [j][r], and after the walk over D a
// row block of B = L^-1, [i][s], then a column block of it, k-major [i][r] -- then each wave's RT
// tiles: tile 0 takes Y[row][j] during the walk, all of them T[row][s] after it, then U = T B^T.
__global__ __launch_bounds__(kLsThreads) void k_lowrank_site_forward_mfma(
    LsOperands a, const float* __restrict__ binv, const double* __restrict__ logterm,
    int64_t groups, float* __restrict__ log_prob, float* __restrict__ coef) {
  extern __shared__ float tiles[];
  __shared__ float ls[kTile], is[kTile], ds[kTile];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int64_t k = blockIdx.x / groups, g = blockIdx.x - k * groups;
  const int64_t N = a.N, D = a.D, R = a.R;
  const int RT = (int)((R + kTile - 1) / kTile);
  float* bs = tiles;
  float* ts = tiles + (RT + w * RT) * kTileFloats;
  const float* W = a.W + k * a.W_sk;
  const float* loc = a.loc + k * a.loc_sk;
  const float* d = a.d + k * a.d_sk;
  const float* x = a.value + k * a.value_sk;
  binv += k * R * R;
  const int64_t ibase = (g * kTileWaves + w) * kTile;
  const bool active = ibase < N;   // (wave-uniform)
  f32x16 acc[kLsMaxRT];
#pragma unroll
  for (int rt = 0; rt < kLsMaxRT; ++rt)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[rt][q] = 0.0f;
  float quad = 0.0f;   // this lane's half of r.y of row `col`
  for (int64_t j0 = 0; j0 < D; j0 += kTile) {
    __syncthreads();   // the previous step's tiles are read
    for (int e = t; e < RT * kTile * kTile; e += kLsThreads) {
      const int rt = e >> 10, jj = (e >> 5) & 31, rr = e & 31;
      const int64_t j = j0 + jj, r = (int64_t)rt * kTile + rr;
      bs[rt * kTileFloats + jj * kTileStride + rr] = (j < D && r < R) ? W[j * R + r] : 0.0f;
    }
    if (t < kTile) {
      const bool ok = j0 + t < D;
      const float dj = ok ? d[j0 + t] : 1.0f;
      ls[t] = ok ? loc[j0 + t] : 0.0f;
      is[t] = ok ? 1.0f / dj : 0.0f;
      ds[t] = ok ? dj : 0.0f;
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 2 * q + half;
        const int64_t i = ibase + row, j = j0 + col;
        ts[row * kTileStride + col] =
            (i < N && j < D) ? (x[i * a.value_si + j] - ls[col]) * is[col] : 0.0f;
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float y = ts[col * kTileStride + 16 * half + c];
        quad = fmaf(y * y, ds[16 * half + c], quad);
      }
#pragma unroll
      for (int rt = 0; rt < kLsMaxRT; ++rt) {
        if (rt < RT) {
#pragma unroll
          for (int s = 0; s < 16; ++s)   // A[row][j] = Y, B[j][r] = W
            acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                ts[col * kTileStride + 2 * s + half],
                tile_k_major(bs + rt * kTileFloats, s, lane), acc[rt], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();   // Y and the last rows of W are read
  if (active) {
#pragma unroll
    for (int rt = 0; rt < kLsMaxRT; ++rt) {
      if (rt < RT) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          ts[rt * kTileFloats + acc_row(q, lane) * kTileStride + col] = acc[rt][q];
      }
    }
  }
  float p[16];   // this lane's 16 rows of sum_i U[row, i]^2, its column of every tile
#pragma unroll
  for (int q = 0; q < 16; ++q) p[q] = 0.0f;
  // U = T B^T, tile by tile into the accumulators T has left
#pragma unroll
  for (int rt = 0; rt < kLsMaxRT; ++rt) {
    if (rt < RT) {   // (block-uniform)
      __syncthreads();   // T is written; the previous row block of B is read
      for (int e = t; e < RT * kTile * kTile; e += kLsThreads) {
        const int st = e >> 10, n = (e >> 5) & 31, kk = e & 31;
        const int64_t ii = (int64_t)rt * kTile + n, ss = (int64_t)st * kTile + kk;
        bs[st * kTileFloats + n * kTileStride + kk] = (ii < R && ss < R) ? binv[ii * R + ss] : 0.0f;
      }
      __syncthreads();
      if (active) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[rt][q] = 0.0f;
        for (int st = 0; st < RT; ++st)   // A[row][s] = T, B[i][s] = L^-1
          mfma_tile_nt(acc[rt], ts + st * kTileFloats, bs + st * kTileFloats, lane);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = fmaf(acc[rt][q], acc[rt][q], p[q]);
      }
    }
  }
  __syncthreads();   // T is read: the wave's tiles now take U
  if (active) {
#pragma unroll
    for (int rt = 0; rt < kLsMaxRT; ++rt) {
      if (rt < RT) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          ts[rt * kTileFloats + acc_row(q, lane) * kTileStride + col] = acc[rt][q];
      }
    }
  }
  // c = U B, a column block of B at a time
  for (int rt = 0; rt < RT; ++rt) {
    __syncthreads();   // U is written; the previous block of B is read
    for (int e = t; e < RT * kTile * kTile; e += kLsThreads) {
      const int st = e >> 10, kk = (e >> 5) & 31, n = e & 31;
      const int64_t ii = (int64_t)st * kTile + kk, rr = (int64_t)rt * kTile + n;
      bs[st * kTileFloats + kk * kTileStride + n] = (ii < R && rr < R) ? binv[ii * R + rr] : 0.0f;
    }
    __syncthreads();
    if (active) {
      f32x16 c;
#pragma unroll
      for (int q = 0; q < 16; ++q) c[q] = 0.0f;
      for (int st = 0; st < RT; ++st) {   // A[row][i] = U, B[i][r] = L^-1, k-major
#pragma unroll
        for (int s = 0; s < 16; ++s)
          c = __builtin_amdgcn_mfma_f32_32x32x2f32(
              ts[st * kTileFloats + col * kTileStride + 2 * s + half],
              tile_k_major(bs + st * kTileFloats, s, lane), c, 0, 0, 0);
      }
      const int64_t r = (int64_t)rt * kTile + col;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t i = ibase + acc_row(q, lane);
        if (i < N && r < R) coef[(k * N + i) * R + r] = c[q];
      }
    }
  }
  __syncthreads();   // the wave's tiles of U are read: tile 0 now takes p
  if (active) {
#pragma unroll
    for (int q = 0; q < 16; ++q) ts[acc_row(q, lane) * kTileStride + col] = p[q];
  }
  __syncthreads();
  if (active) {
    float u = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c) u += ts[col * kTileStride + 16 * half + c];
    quad += __shfl_xor(quad, 32, kWave);
    u += __shfl_xor(u, 32, kWave);
    const int64_t i = ibase + col;
    if (half == 0 && i < N)
      log_prob[k * N + i] = (float)(-0.5 * (logterm[k] + ((double)quad - (double)u)));
  }
}

// ---- the backward row pass: a workgroup per (particle, slice of rows, 32 columns of D) -----------
// Thread (tx, ty) of 32 x 8: in phase A column j = 32 jt + tx of rows ty, ty + 8, ... of the 32 staged
// rows; in phase B the entries [j][ty + 8 u], u < RU, of the slice's g a c^T. LDS rows of R | 1 floats
// (odd: conflict-free along tx).
struct LsPartials {
  float* g;     // [K][S]
  float* loc;   // [K][S][D]
  float* d;     // [K][S][D]
  float* W;     // [K][S][D][R]
};

template <int RU>
__global__ __launch_bounds__(kLsThreads) void k_lowrank_site_backward(
    LsOperands a, const float* __restrict__ coef, const float* __restrict__ g, int64_t g_sk,
    int64_t g_si, int64_t S, int64_t rows, int want_loc, int want_W, int want_d,
    float* __restrict__ dvalue, LsPartials part) {
  extern __shared__ float lds[];
  __shared__ float gsh[kTile];
  __shared__ float red_loc[8][kTile], red_d[8][kTile], red_g[8];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int64_t N = a.N, D = a.D, R = a.R;
  const int64_t DT = (D + kTile - 1) / kTile;
  const int64_t jt = blockIdx.x % DT, s = (blockIdx.x / DT) % S, k = blockIdx.x / (DT * S);
  const int ld = (int)R | 1;
  float* ws = lds;
  float* cs = lds + kTile * ld;
  float* gs = cs + kTile * ld;
  const float* W = a.W + k * a.W_sk;
  const float* x = a.value + k * a.value_sk;
  for (int e = t; e < kTile * (int)R; e += kLsThreads) {
    const int jj = e / (int)R, r = e - jj * (int)R;
    const int64_t j = jt * kTile + jj;
    ws[jj * ld + r] = j < D ? W[j * R + r] : 0.0f;
  }
  const int64_t j = jt * kTile + tx;
  const bool jok = j < D;
  const float lj = jok ? a.loc[k * a.loc_sk + j] : 0.0f;
  const float ij = jok ? 1.0f / a.d[k * a.d_sk + j] : 0.0f;
  float acc[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) acc[u] = 0.0f;
  float sloc = 0.0f, sd = 0.0f, sg = 0.0f;
  const int64_t i0 = s * rows, i1 = min(N, i0 + rows);
  for (int64_t ib = i0; ib < i1; ib += kTile) {
    __syncthreads();   // the previous rows are read
    if (t < kTile) gsh[t] = ib + t < i1 ? g[k * g_sk + (ib + t) * g_si] : 0.0f;
    __syncthreads();
    for (int e = t; e < kTile * (int)R; e += kLsThreads) {
      const int row = e / (int)R, r = e - row * (int)R;
      cs[row * ld + r] = gsh[row] != 0.0f ? coef[(k * N + ib + row) * R + r] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = ty + 8 * v;
      const int64_t i = ib + row;
      const float gi = gsh[row];
      float ga = 0.0f;
      if (gi != 0.0f && jok) {
        float P = 0.0f;
        for (int r = 0; r < (int)R; ++r) P = fmaf(cs[row * ld + r], ws[tx * ld + r], P);
        const float aij = (x[i * a.value_si + j] - lj - P) * ij;
        ga = gi * aij;
        sloc += ga;
        sd = fmaf(ga, aij, sd);
      }
      if (dvalue != nullptr && jok && i < i1) dvalue[(k * N + i) * D + j] = gi != 0.0f ? -ga : 0.0f;
      gs[row * kTileStride + tx] = ga;
      if (tx == 0) sg += gi;
    }
    __syncthreads();
    if (want_W) {
#pragma unroll 4   // (unrolled whole, the RU = 8 kernel takes every register: one wave per SIMD)
      for (int row = 0; row < kTile; ++row) {
        const float gv = gs[row * kTileStride + tx];
#pragma unroll
        for (int u = 0; u < RU; ++u)
          acc[u] = fmaf(gv, cs[row * ld + min(ty + 8 * u, (int)R - 1)], acc[u]);
      }
    }
  }
  red_loc[ty][tx] = sloc;
  red_d[ty][tx] = sd;
  if (tx == 0) red_g[ty] = sg;
  __syncthreads();
  const int64_t base = (k * S + s) * D + j;
  if (ty == 0 && jok) {
    float l = 0.0f, q = 0.0f;
#pragma unroll
    for (int v = 0; v < 8; ++v) l += red_loc[v][tx], q += red_d[v][tx];
    if (want_loc) part.loc[base] = l;
    if (want_d) part.d[base] = q;
  }
  if (t == 0 && jt == 0) {
    float q = 0.0f;
#pragma unroll
    for (int v = 0; v < 8; ++v) q += red_g[v];
    part.g[k * S + s] = q;
  }
  if (want_W && jok) {
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (ty + 8 * u < R) part.W[base * R + ty + 8 * u] = acc[u];
  }
}

// ---- the finish: a workgroup per (particle, row j of W), thread r ----------------------------------
__global__ __launch_bounds__(kLsFinishThreads) void k_lowrank_site_finish(
    LsOperands a, const float* __restrict__ binv, int64_t S, LsPartials part,
    float* __restrict__ dloc, float* __restrict__ dW, float* __restrict__ dd) {
  __shared__ float wj[kLsFinishThreads], vj[kLsFinishThreads], mw[kLsFinishThreads];
  const int r = threadIdx.x;
  const int64_t D = a.D, R = a.R;
  const int64_t k = blockIdx.x / D, j = blockIdx.x - k * D;
  if (dloc != nullptr && r == 0) {
    float l = 0.0f;
    for (int64_t s = 0; s < S; ++s) l += part.loc[(k * S + s) * D + j];
    dloc[k * D + j] = l;
  }
  if (dW == nullptr && dd == nullptr) return;   // (block-uniform)
  float G = 0.0f;
  for (int64_t s = 0; s < S; ++s) G += part.g[k * S + s];
  wj[r] = r < R ? a.W[k * a.W_sk + j * R + r] : 0.0f;
  __syncthreads();
  binv += k * R * R;
  float v = 0.0f;   // (B W_j)[r]
  if (r < R)
    for (int64_t s = 0; s <= r; ++s) v = fmaf(binv[r * R + s], wj[s], v);
  vj[r] = v;
  __syncthreads();
  float m = 0.0f;   // M[j][r] = (B^T B W_j)[r]
  if (r < R)
    for (int64_t i = r; i < R; ++i) m = fmaf(vj[i], binv[i * R + r], m);
  const float inv = 1.0f / a.d[k * a.d_sk + j];
  if (dW != nullptr && r < R) {
    float acc = 0.0f;
    for (int64_t s = 0; s < S; ++s) acc += part.W[((k * S + s) * D + j) * R + r];
    dW[(k * D + j) * R + r] = acc - G * (m * inv);
  }
  if (dd == nullptr) return;
  mw[r] = m * wj[r];
  __syncthreads();
  if (r == 0) {
    float q = 0.0f, acc = 0.0f;
    for (int64_t c = 0; c < R; ++c) q += mw[c];
    for (int64_t s = 0; s < S; ++s) acc += part.d[(k * S + s) * D + j];
    dd[k * D + j] = 0.5f * acc - 0.5f * G * (inv - q * inv * inv);
  }
}

}  // namespace mi

namespace {

constexpr int64_t kFill = 1024;            // blocks that fill the chip (256 CUs, a few each)
constexpr size_t kStaticLds = 64 * 1024;   // what a launch may ask for without saying so first

int ls_check_shape(int64_t K, int64_t N, int64_t D, int64_t R) {
  if (K < 1 || N < 1 || D < 1 || R < 1) return MI_EINVAL;
  if (D > MI_LOWRANK_SITE_MAX_D || R > MI_LOWRANK_MAX_R) return MI_EUNSUPPORTED;
  // grids are one-dimensional: the particles times the rows' tiles, and the particles times D
  if (K > kMaxGrid / D || K > kMaxGrid / ceil_div(N, mi::kTile)) return MI_EUNSUPPORTED;
  return 0;
}

// the backward's slices of rows: enough workgroups to fill the chip, whole tiles of 32 rows
struct LsSlices {
  int64_t S, rows;
};

LsSlices ls_slices(int64_t K, int64_t N, int64_t D) {
  const int64_t DT = ceil_div(D, mi::kTile);
  int64_t S = std::max<int64_t>(1, std::min(ceil_div(kFill, K * DT), ceil_div(N, mi::kTile)));
  LsSlices g{};
  g.rows = ceil_div(ceil_div(N, S), mi::kTile) * mi::kTile;
  g.S = ceil_div(N, g.rows);
  return g;
}

// workspace: the K log terms (fp64), L^-1 (K R R floats, padded to 8 bytes), then the backward's
// partials g [K][S], loc [K][S][D], d [K][S][D] and W [K][S][D][R]
size_t ls_binv_bytes(int64_t K, int64_t R) {
  return ((size_t)(K * R * R) * sizeof(float) + 7) & ~(size_t)7;
}

size_t ls_workspace_bytes(int64_t K, int64_t N, int64_t D, int64_t R) {
  const LsSlices g = ls_slices(K, N, D);
  return sizeof(double) * (size_t)K + ls_binv_bytes(K, R) +
         sizeof(float) * (size_t)(K * g.S) * (size_t)(1 + D * (2 + R));
}

template <typename Kernel>
hipError_t ls_allow_lds(Kernel kernel, size_t bytes) {
  if (bytes <= kStaticLds) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

int ls_capacitance(const float* L, int64_t L_sk, const float* d, int64_t d_sk, int64_t K,
                   int64_t D, int64_t R, float* binv, double* logterm, hipStream_t s) {
  const int n = (int)R;
  const size_t lds = sizeof(double) * (size_t)(n * (n | 1) + 1024 / mi::kWave);
  const hipError_t e = ls_allow_lds(mi::k_lowrank_site_capacitance, lds);
  if (e != hipSuccess) return to_code(e);
  hipLaunchKernelGGL(mi::k_lowrank_site_capacitance, dim3((unsigned)K), dim3(n <= 32 ? 256 : 1024),
                     lds, s, L, L_sk, d, d_sk, n, D, binv, logterm);
  return to_code(hipGetLastError());
}

}  // namespace

extern "C" {

int mi_lowrank_site_workspace_bytes(int64_t K, int64_t N, int64_t D, int64_t R, size_t* bytes) {
  const int bad = ls_check_shape(K, N, D, R);
  if (bad != 0) return bad;
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = ls_workspace_bytes(K, N, D, R);
  return 0;
}

int mi_lowrank_site_forward(const float* value, int64_t value_stride_k, int64_t value_stride_i,
                            const float* loc, int64_t loc_stride_k, const float* cov_factor,
                            int64_t cov_factor_stride_k, const float* cov_diag,
                            int64_t cov_diag_stride_k, const float* capacitance_tril,
                            int64_t capacitance_tril_stride_k, int64_t K, int64_t N, int64_t D,
                            int64_t R, void* workspace, size_t workspace_bytes, float* log_prob,
                            float* coef, void* stream) {
  const int bad = ls_check_shape(K, N, D, R);
  if (bad != 0) return bad;
  if (value == nullptr || loc == nullptr || cov_factor == nullptr || cov_diag == nullptr ||
      capacitance_tril == nullptr || log_prob == nullptr || coef == nullptr ||
      workspace == nullptr || workspace_bytes < ls_workspace_bytes(K, N, D, R))
    return MI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* logterm = static_cast<double*>(workspace);
  float* binv = reinterpret_cast<float*>(logterm + K);
  const mi::LsOperands a{value, value_stride_k, value_stride_i, loc, loc_stride_k, cov_factor,
                         cov_factor_stride_k, cov_diag, cov_diag_stride_k, K, N, D, R};
  int code = ls_capacitance(capacitance_tril, capacitance_tril_stride_k, cov_diag,
                            cov_diag_stride_k, K, D, R, binv, logterm, s);
  if (code != 0) return code;
  if (R >= mi::kTile) {
    const int64_t groups = ceil_div(N, (int64_t)mi::kTile * mi::kTileWaves);
    const int64_t RT = ceil_div(R, mi::kTile);
    const size_t lds = sizeof(float) * (size_t)((1 + mi::kTileWaves) * RT * mi::kTileFloats);
    const hipError_t e = ls_allow_lds(mi::k_lowrank_site_forward_mfma, lds);
    if (e != hipSuccess) return to_code(e);
    hipLaunchKernelGGL(mi::k_lowrank_site_forward_mfma, dim3((unsigned)(K * groups)),
                       dim3(mi::kLsThreads), lds, s, a, binv, logterm, groups, log_prob, coef);
  } else {
    const int64_t tiles = ceil_div(N, mi::kLsThreads);
    const dim3 grid((unsigned)(K * tiles));
#define MI_LS_ROWS(RP)                                                                         \
  hipLaunchKernelGGL(mi::k_lowrank_site_forward_valu<RP>, grid, dim3(mi::kLsThreads), 0, s, a, \
                     binv, logterm, tiles, log_prob, coef)
    if (R <= 4) MI_LS_ROWS(4);
    else if (R <= 8) MI_LS_ROWS(8);
    else if (R <= 16) MI_LS_ROWS(16);
    else MI_LS_ROWS(32);
#undef MI_LS_ROWS
  }
  return to_code(hipGetLastError());
}

int mi_lowrank_site_backward(const float* g, int64_t g_stride_k, int64_t g_stride_i,
                             const float* value, int64_t value_stride_k, int64_t value_stride_i,
                             const float* loc, int64_t loc_stride_k, const float* cov_factor,
                             int64_t cov_factor_stride_k, const float* cov_diag,
                             int64_t cov_diag_stride_k, const float* capacitance_tril,
                             int64_t capacitance_tril_stride_k, const float* coef, int64_t K,
                             int64_t N, int64_t D, int64_t R, void* workspace,
                             size_t workspace_bytes, float* dvalue, float* dloc,
                             float* dcov_factor, float* dcov_diag, void* stream) {
  const int bad = ls_check_shape(K, N, D, R);
  if (bad != 0) return bad;
  if (g == nullptr || value == nullptr || loc == nullptr || cov_factor == nullptr ||
      cov_diag == nullptr || capacitance_tril == nullptr || coef == nullptr ||
      workspace == nullptr || workspace_bytes < ls_workspace_bytes(K, N, D, R))
    return MI_EINVAL;
  if (dvalue == nullptr && dloc == nullptr && dcov_factor == nullptr && dcov_diag == nullptr)
    return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LsSlices sl = ls_slices(K, N, D);
  double* logterm = static_cast<double*>(workspace);
  float* binv = reinterpret_cast<float*>(logterm + K);
  mi::LsPartials part{};
  part.g = reinterpret_cast<float*>(reinterpret_cast<char*>(binv) + ls_binv_bytes(K, R));
  part.loc = part.g + K * sl.S;
  part.d = part.loc + K * sl.S * D;
  part.W = part.d + K * sl.S * D;
  const mi::LsOperands a{value, value_stride_k, value_stride_i, loc, loc_stride_k, cov_factor,
                         cov_factor_stride_k, cov_diag, cov_diag_stride_k, K, N, D, R};
  const bool factor = dcov_factor != nullptr || dcov_diag != nullptr;
  if (factor) {
    const int code = ls_capacitance(capacitance_tril, capacitance_tril_stride_k, cov_diag,
                                    cov_diag_stride_k, K, D, R, binv, logterm, s);
    if (code != 0) return code;
  }
  const int64_t DT = ceil_div(D, mi::kTile);
  const dim3 grid((unsigned)(K * sl.S * DT));
  const size_t lds = sizeof(float) * (size_t)(2 * mi::kTile * (R | 1) + mi::kTileFloats);
#define MI_LS_BACKWARD(RU)                                                                      \
  hipLaunchKernelGGL(mi::k_lowrank_site_backward<RU>, grid, dim3(mi::kLsThreads), lds, s, a,    \
                     coef, g, g_stride_k, g_stride_i, sl.S, sl.rows, (int)(dloc != nullptr),    \
                     (int)(dcov_factor != nullptr), (int)(dcov_diag != nullptr), dvalue, part)
  if (R <= 8) MI_LS_BACKWARD(1);
  else if (R <= 16) MI_LS_BACKWARD(2);
  else if (R <= 32) MI_LS_BACKWARD(4);
  else if (R <= 64) MI_LS_BACKWARD(8);
  else MI_LS_BACKWARD(16);
#undef MI_LS_BACKWARD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  if (dloc == nullptr && !factor) return 0;
  hipLaunchKernelGGL(mi::k_lowrank_site_finish, dim3((unsigned)(K * D)),
                     dim3(mi::kLsFinishThreads), 0, s, a, binv, sl.S, part, dloc, dcov_factor,
                     dcov_diag);
  return to_code(hipGetLastError());
}

}  // extern "C"
