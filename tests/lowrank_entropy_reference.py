"""
The yardstick of the native LowRankMultivariateNormal entropy (mi_lowrank_entropy): its closed form
and that of its gradient in float64 numpy, from the float32 inputs the kernel reads, and the inputs
every case is made of.

With W = cov_factor [D, R], d = cov_diag [D], C = I + W^T diag(1 / d) W = L L^T and M = W C^-1:
  H         = 0.5 D (1 + log 2 pi) + sum_j log L[j, j] + 0.5 sum_i log d[i]
  dH/dW[i, r] = M[i, r] / d[i]
  dH/dd[i]    = 0.5 (1 / d[i] - (sum_r M[i, r] W[i, r]) / d[i]^2)
L is the factor the kernel is handed (float32 values), of which only the lower triangle counts.
"""
import math

import numpy as np


def inputs(D, R, seed):
    """W = 0.3 N(0, 1), d uniform in [0.5, 2] and L = the float64 Cholesky factor of
    I + W^T diag(1 / d) W rounded to float32: float32 values held in float64."""
    rng = np.random.default_rng(seed)
    W = (0.3 * rng.standard_normal((D, R))).astype(np.float32).astype(np.float64)
    d = (0.5 + 1.5 * rng.random(D)).astype(np.float32).astype(np.float64)
    C = np.eye(R) + W.T @ (W / d[:, None])
    L = np.linalg.cholesky(C).astype(np.float32).astype(np.float64)
    return W, d, L


def case_seed(D, R):
    return 100000 + 1000 * R + D


def closed_form(W, d, L):
    """(H, dH/dW, dH/dd, C^-1) in float64."""
    D, R = W.shape
    L = np.tril(L)
    Linv = np.linalg.solve(L, np.eye(R))
    Cinv = Linv.T @ Linv
    M = W @ Cinv
    H = 0.5 * D * (1.0 + math.log(2.0 * math.pi)) + np.log(np.diag(L)).sum() + \
        0.5 * np.log(d).sum()
    dW = M / d[:, None]
    dd = 0.5 * (1.0 / d - (M * W).sum(1) / d ** 2)
    return H, dW, dd, Cinv
