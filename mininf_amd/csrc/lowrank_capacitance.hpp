// The R x R stage the LowRankMultivariateNormal entropy (lowrank_entropy.hip) and site density
// (lowrank_site.hip) share: L^-1, and C^-1 = L^-T L^-1, from the capacitance factor L, by one
// workgroup in fp64.
//
// One fp64 array X[R][ld] (ld = R | 1, odd: rows and columns both conflict-free) carries everything:
// at the start its strict upper triangle holds L^T (X[k][i] = L[i][k], i > k), its diagonal
// 1 / L[k][k] and its strict lower triangle the right-hand side I (zeros: the unit diagonal is
// implied). Step k reads only row k -- the unscaled row k of L^-1 to its left, column k of L to its
// right -- and updates the rows below it, so one barrier separates the steps.
#pragma once

#include "common.hpp"

namespace mi {

// X from the lower triangle of L[R][R]; the caller's barrier follows.
MI_DEV void capacitance_stage(const float* __restrict__ L, int R, double* X) {
  const int ld = R | 1;
  for (int e = threadIdx.x; e < R * R; e += blockDim.x) {
    const int r = e / R, c = e - r * R;
    if (c < r) {
      X[c * ld + r] = (double)L[e];
      X[r * ld + c] = 0.0;
    } else if (c == r) {
      X[r * ld + r] = 1.0 / (double)L[e];
    }
  }
}

// X = L^-1 (zero above the diagonal) from the staged X, by the whole workgroup (a multiple of 64
// threads); a barrier has followed the last write.
MI_DEV void capacitance_factor_inverse(double* X, int R) {
  const int ld = R | 1;
  const int t = threadIdx.x, nt = blockDim.x;
  const int tx = t & (kWave - 1), ty = t >> 6, ny = nt >> 6;
  for (int k = 0; k + 1 < R; ++k) {
    const double rk = X[k * ld + k];
    for (int j = tx; j <= k; j += kWave) {
      const double xk = j == k ? rk : X[k * ld + j] * rk;   // L^-1[k][j]
      for (int i = k + 1 + ty; i < R; i += ny)
        X[i * ld + j] = fma(-X[k * ld + i], xk, X[i * ld + j]);
    }
    __syncthreads();
  }
  // the rows scaled: X = L^-1, zero above the diagonal
  for (int e = t; e < R * R; e += nt) {
    const int i = e / R, j = e - i * R;
    if (j < i) X[i * ld + j] *= X[i * ld + i];
    else if (j > i) X[i * ld + j] = 0.0;
  }
  __syncthreads();
}

// cinv[R][R] = C^-1 = L^-T L^-1 (f32, full and exactly symmetric) from the staged X; X is consumed.
MI_DEV void capacitance_invert(double* X, int R, float* __restrict__ cinv) {
  capacitance_factor_inverse(X, R);
  const int ld = R | 1;
  const int t = threadIdx.x, nt = blockDim.x;
  const int tx = t & (kWave - 1), ty = t >> 6, ny = nt >> 6;
  // C^-1[a][b] = sum_i X[i][a] X[i][b], i ascending (the terms with i < max(a, b) are zeros, so
  // [a][b] and [b][a] are the same sum)
  for (int a0 = ty * 8; a0 < R; a0 += ny * 8) {
    for (int b = tx; b < R; b += kWave) {
      double acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = 0.0;
      for (int i = a0; i < R; ++i) {
        const double xb = X[i * ld + b];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fma(X[i * ld + min(a0 + u, R - 1)], xb, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (a0 + u < R) cinv[(a0 + u) * R + b] = (float)acc[u];
    }
  }
}

}  // namespace mi
