"""
The fp64 reference and the launch helper of the count regressions of the linear-predictor site
kernels (mi_linear_forward with MI_POISSON, MI_BINOMIAL, MI_NEGATIVE_BINOMIAL), shared by
test_count_linear_host.py and test_gpu_count_linear.py. Geometry, the folded prior and the poisoned
buffers are those of linear_reference.py.

reference():    with eta = X @ theta in fp64,
                  Poisson            y eta - exp(eta) - lgamma(y + 1)
                  Binomial           y eta - n softplus(eta) + lgamma(n + 1) - lgamma(y + 1) - lgamma(n - y + 1)
                  NegativeBinomial   r logsigmoid(-eta) + y logsigmoid(eta) + lgamma(r + y) - lgamma(1 + y)
                                     - lgamma(r), the lgamma terms 0 where r + y == 0
                (poisson.py:60-65, binomial.py:140-158, negative_binomial.py:130-150) and
                d/d eta = y - exp(eta), y - n sigmoid(eta), y - (y + r) sigmoid(eta). Returns
                (total [K], dtheta [K, P], bound [K, P], tbound [K]): bound is the sum of the absolute
                values of the terms of dtheta / g0, tbound the sum over rows of the absolute values of
                the log density's separate parts.
float32_restatement(): the kernels' formula in float32 numpy (csrc/linear.hip, "count regressions"),
                eta a float32 fmaf chain, row sums in fp64: what the tolerances are checked against
                before a GPU run.
launch(), run(): linear_reference.launch() with the count operand.
"""
import ctypes
from math import lgamma as _lgamma

import numpy as np

from tests.linear_reference import (GUARD, PARTICLE_CHUNK, Result, geometry, mfma_eligible, prior_terms)
from mininf_amd import _native as nat

FAMILIES = {"poisson": nat.POISSON, "binomial": nat.BINOMIAL,
            "negative_binomial": nat.NEGATIVE_BINOMIAL}

lgamma = np.vectorize(_lgamma, otypes=[np.float64])


def _softplus(x):
    return np.logaddexp(0.0, x)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def row_constant(family, y, n):
    """(c [N], |parts| of c [N]) in fp64: the terms of a row alone."""
    if family == nat.POISSON:
        c = -lgamma(y + 1)
        return c, np.abs(c)
    if family == nat.BINOMIAL:
        parts = [lgamma(n + 1), -lgamma(y + 1), -lgamma(n - y + 1)]
    else:
        point = (n + y) == 0
        safe_n = np.where(point, 1.0, n)
        parts = [np.where(point, 0.0, lgamma(safe_n + y)), np.where(point, 0.0, -lgamma(1 + y)),
                 np.where(point, 0.0, -lgamma(safe_n))]
    return sum(parts), sum(np.abs(p) for p in parts)


def reference(family, X, theta, y, mask, count, site_scale, g0, row_index=None, prior=None):
    if row_index is not None:
        X, y, mask, count = X[row_index], y[row_index], mask[row_index], count[row_index]
    X64 = X.astype(np.float64)
    absX = np.abs(X64)
    m = mask.astype(np.float64)[:, None]
    y1 = np.where(mask, y, 0.0).astype(np.float64)     # masked lanes are never read
    n1 = np.where(mask, count, 1.0).astype(np.float64)
    c, cabs = row_constant(family, y1, n1)
    y64, n64 = y1[:, None], n1[:, None]
    K, P = theta.shape
    total, tbound = np.empty(K), np.empty(K)
    dtheta, bound = np.empty((K, P)), np.empty((K, P))
    for k0 in range(0, K, PARTICLE_CHUNK):
        k1 = min(K, k0 + PARTICLE_CHUNK)
        th = theta[k0:k1].astype(np.float64)
        eta = X64 @ th.T
        if family == nat.POISSON:
            parts = [y64 * eta, -np.exp(eta)]
            deta = y64 - np.exp(eta)
        elif family == nat.BINOMIAL:
            parts = [y64 * eta, -n64 * _softplus(eta)]
            deta = y64 - n64 * _sigmoid(eta)
        else:
            parts = [-n64 * _softplus(eta), -y64 * _softplus(-eta)]
            deta = y64 - (y64 + n64) * _sigmoid(eta)
        lp = sum(parts) + c[:, None]
        total[k0:k1] = site_scale * (m * lp).sum(0)
        tbound[k0:k1] = abs(site_scale) * (m * (sum(np.abs(p) for p in parts) + cabs[:, None])).sum(0)
        dtheta[k0:k1] = g0 * site_scale * ((m * deta).T @ X64)
        bound[k0:k1] = site_scale * (np.abs(m * deta).T @ absX) + 1e-6
        if prior is not None:
            plp, pd = prior_terms(prior, th)
            total[k0:k1] += prior.scale * plp.sum(1)
            tbound[k0:k1] += np.abs(prior.scale * plp).sum(1)
            dtheta[k0:k1] += g0 * prior.scale * pd
            bound[k0:k1] += np.abs(prior.scale * pd)
    return total, dtheta, bound, tbound


def float32_restatement(family, X, theta, y, mask, count, site_scale, g0, row_index=None,
                        prior=None):
    """
    (total [K], dtheta [K, P]) by the kernels' float32 formula: eta as the float32 fmaf chain over
    the features in order (what v_mfma_f32_32x32x2_f32 and the VALU kernel's fmaf compute), the
    elementwise step in float32, the sums over rows in fp64, the folded prior in fp64.
    """
    f = np.float32
    if row_index is not None:
        X, y, mask, count = X[row_index], y[row_index], mask[row_index], count[row_index]
    m = mask.astype(bool)
    y32 = np.where(m, y, 0).astype(f)[:, None]
    n32 = np.where(m, count, 0).astype(f)[:, None]
    eta = np.zeros((X.shape[0], theta.shape[0]), f)
    for j in range(X.shape[1]):   # one rounding per step: the product is exact in fp64
        eta = (eta.astype(np.float64) +
               X[:, j].astype(np.float64)[:, None] * theta[:, j].astype(np.float64)[None, :]).astype(f)
    c, _ = row_constant(family, np.where(m, y, 0.0).astype(np.float64),
                        np.where(m, count, 1.0).astype(np.float64))
    c = np.where(m, c.astype(f), f(0)).astype(np.float64)
    if family == nat.POISSON:
        e = np.where(m[:, None], np.exp(eta), f(0)).astype(f)
        lp = (y32 * eta).astype(f) - e
        d = y32 - e
    else:
        if family == nat.BINOMIAL:
            t, a = n32, y32 - n32
        else:
            t, a = (n32 + y32).astype(f), -n32
        e = np.exp(-np.abs(eta)).astype(f)
        u = (f(1) + e).astype(f)
        l1p = np.log1p(e).astype(f)
        sig = np.where(eta >= 0, f(1) / u, e / u).astype(f)
        lp = (np.where(eta >= 0, a, y32) * eta).astype(f) - (t * l1p).astype(f)
        d = (y32 - (t * sig).astype(f)).astype(f)
    total = site_scale * (lp.astype(np.float64).sum(0) + c.sum())
    dtheta = g0 * site_scale * (np.where(m[:, None], d, 0).astype(np.float64).T @ X.astype(np.float64))
    if prior is not None:
        plp, pd = prior_terms(prior, theta.astype(np.float64))
        total = total + prior.scale * plp.sum(1)
        dtheta = dtheta + g0 * prior.scale * pd
    return total, dtheta


def launch(family, X, theta, y, mask, count, site_scale, g0, valu, compute_grads=1,
           row_index=None, prior=None):
    """
    One mi_linear_forward of a count regression over poisoned buffers (linear_reference.launch).
    count: a device tensor (its stride goes to the site), a float (the constant) or None (Poisson).
    """
    import torch
    device = X.device
    P = X.shape[1]
    N = X.shape[0] if row_index is None else row_index.shape[0]
    K = theta.shape[0]
    L = nat.Linear()
    L.K, L.N, L.P = K, N, P
    L.family = family
    L.options = nat.LINEAR_VALU if valu else 0
    L.x = X.data_ptr()
    L.x_stride_i, L.x_stride_j = X.stride()
    L.theta = theta.data_ptr()
    L.theta_stride_k, L.theta_stride_j = theta.stride()
    L.value = y.data_ptr()
    L.value_stride_i = y.stride(0)
    if mask is not None:
        L.mask = mask.data_ptr()
        L.mask_stride_i = mask.stride(0)
    if isinstance(count, torch.Tensor):
        L.count = count.data_ptr()
        L.count_stride_i = count.stride(0)
    elif count is not None:
        L.count_constant = float(count)
    L.grad_scale = g0
    L.site_scale = site_scale
    L.compute_grads = compute_grads
    if row_index is not None:
        assert row_index.dtype == torch.int32 and row_index.is_contiguous()
        L.row_index = row_index.data_ptr()
    flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    prior_flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    if prior is not None:
        L.prior.present = 1
        L.prior.family = prior.family
        L.prior.constant[0], L.prior.constant[1] = prior.c0, prior.c1
        L.prior.scale = prior.scale
        L.prior.flags = prior_flags.data_ptr()
    geo = geometry(N, P, K, False, prior is not None,
                   mfma_eligible(P, L.x_stride_i, L.x_stride_j, L.x, valu))
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "workspace")
    assert size.value == geo.workspace_bytes, (size.value, vars(geo))
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    total = torch.full((K,), float("nan"), device=device)
    dslots = torch.full((P, K), float("nan"), device=device)
    rc = lib.mi_linear_forward(ctypes.byref(L), work.data_ptr() + GUARD, size.value,
                               total.data_ptr(), dslots.data_ptr(), flags.data_ptr(),
                               nat.stream_handle(device))
    torch.cuda.synchronize()
    assert bool((work[:GUARD] == 0xFF).all()), "the launch wrote below its workspace"
    assert bool((work[GUARD + size.value:] == 0xFF).all()), "the launch wrote past its workspace"
    if not compute_grads or rc != 0:
        assert bool(torch.isnan(dslots).all()), "dslots written without compute_grads"
    return Result(rc, total.cpu().numpy(), dslots.cpu().numpy(),
                  int(flags.cpu()[0]) & 0xFFFFFFFF, int(prior_flags.cpu()[0]) & 0xFFFFFFFF, geo)


def run(family, X, theta, y, mask, count, site_scale, g0, valu, **options):
    r = launch(family, X, theta, y, mask, count, site_scale, g0, valu, **options)
    nat.check(r.rc, "mi_linear_forward")
    return r.total, r.dslots, r.flags
