"""
NumPy float64 restatement of the LowRankMultivariateNormal site (csrc/lowrank_site.hip,
include/mininf_amd.h mi_lowrank_site_forward / mi_lowrank_site_backward), with the inputs
tests/test_gpu_lowrank_site.py and tests/test_lowrank_site_host.py share.

Per particle k and row i, with r = x_i - loc, y = r / d, C = I + W^T diag(1 / d) W = L L^T,
t = W^T y and c = C^-1 t:
    log_prob = -1/2 (D log 2 pi + 2 sum_j log L_jj + sum_j log d_j + r.y - t.c)
and for an upstream g[k, i], a_i = (r_i - W c_i) / d, G = sum_i g_i, M = W C^-1:
    dvalue = -g_i a_i, dloc = sum_i g_i a_i, dcov_factor = sum_i g_i a_i c_i^T - G M / d[:, None],
    dcov_diag_j = 1/2 sum_i g_i a_ij^2 - 1/2 G (1 / d_j - (sum_r M_jr W_jr) / d_j^2).
"""
import itertools

import numpy as np

LOG_2PI = np.log(2.0 * np.pi)
NAMES = ("log_prob", "dvalue", "dloc", "dcov_factor", "dcov_diag")
GRADS = NAMES[1:]


def closed_form(value, loc, cov_factor, cov_diag, g):
    """
    The site in float64 for value [K or 1, N, D], loc [K or 1, D], cov_factor [K or 1, D, R],
    cov_diag [K or 1, D] and the upstream g [K, N]. Returns a dict of ``log_prob`` [K, N], ``coef``
    [K, N, R], ``dvalue`` [K, N, D], ``dloc`` [K, D], ``dcov_factor`` [K, D, R], ``dcov_diag`` [K, D]
    (each per particle: a shared parameter's gradient is their sum over k), and ``<name>_size``:
    the sum of the absolute terms of each entry's formula, which the errors are relative to.
    """
    x, loc, W, d, g = (np.asarray(a, np.float64) for a in (value, loc, cov_factor, cov_diag, g))
    K = g.shape[0]
    x = np.broadcast_to(x, (K,) + x.shape[1:])
    loc = np.broadcast_to(loc, (K,) + loc.shape[1:])
    W = np.broadcast_to(W, (K,) + W.shape[1:])
    d = np.broadcast_to(d, (K,) + d.shape[1:])
    D, R = W.shape[1:]
    C = np.eye(R) + np.einsum("kjr,kj,kjs->krs", W, 1.0 / d, W)
    L = np.linalg.cholesky(C)
    Cinv = np.linalg.inv(C)
    logL = np.log(np.diagonal(L, axis1=1, axis2=2))
    with np.errstate(invalid="ignore"):
        r = x - loc[:, None, :]
        y = r / d[:, None, :]
        t = np.einsum("kij,kjr->kir", y, W)
        c = np.einsum("kis,ksr->kir", t, Cinv)
        ry, tc = (r * y).sum(-1), (t * c).sum(-1)
        out = {"coef": c, "L": L}
        out["log_prob"] = -0.5 * (D * LOG_2PI + 2.0 * logL.sum(-1)[:, None] +
                                  np.log(d).sum(-1)[:, None] + ry - tc)
        out["log_prob_size"] = 0.5 * (D * LOG_2PI + 2.0 * np.abs(logL).sum(-1)[:, None] +
                                      np.abs(np.log(d)).sum(-1)[:, None] + ry + tc)
        Wc = np.einsum("kjr,kir->kij", W, c)
        a = (r - Wc) / d[:, None, :]
        A = (np.abs(r) + np.einsum("kjr,kir->kij", np.abs(W), np.abs(c))) / d[:, None, :]
    # a row of zero upstream contributes exact zeros, whatever its value holds
    on = (g != 0)[:, :, None]
    a, A, c0 = np.where(on, a, 0.0), np.where(on, A, 0.0), np.where(on, c, 0.0)
    ga, gA = g[:, :, None] * a, np.abs(g)[:, :, None] * A
    G, Gabs = g.sum(1), np.abs(g).sum(1)
    M = np.einsum("kjs,ksr->kjr", W, Cinv)
    Mabs = np.einsum("kjs,ksr->kjr", np.abs(W), np.abs(Cinv))
    inv = 1.0 / d
    out["dvalue"], out["dvalue_size"] = -ga, gA
    out["dloc"], out["dloc_size"] = ga.sum(1), gA.sum(1)
    out["dcov_factor"] = np.einsum("kij,kir->kjr", ga, c0) - \
        G[:, None, None] * M * inv[:, :, None]
    out["dcov_factor_size"] = np.einsum("kij,kir->kjr", gA, np.abs(c0)) + \
        Gabs[:, None, None] * Mabs * inv[:, :, None]
    out["dcov_diag"] = 0.5 * (ga * a).sum(1) - \
        0.5 * G[:, None] * (inv - (M * W).sum(-1) * inv * inv)
    out["dcov_diag_size"] = 0.5 * (gA * A).sum(1) + \
        0.5 * Gabs[:, None] * (inv + (Mabs * np.abs(W)).sum(-1) * inv * inv)
    return out


def fractions(got, want, rows=None):
    """Largest error of each quantity of ``got`` (those that are not None) over its size in
    ``want``; entries of size 0 must be exact zeros. ``rows`` [K, N] (bool) restricts log_prob to
    the rows that count (a masked row's density may be anything)."""
    out = {}
    for name in NAMES:
        if got.get(name) is None:
            continue
        g, w, size = np.asarray(got[name], np.float64), want[name], want[name + "_size"]
        if name == "log_prob" and rows is not None:
            g, w, size = g[rows], w[rows], size[rows]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert not np.isnan(g).any(), name
        err = np.abs(g - w)
        assert np.all(err[size == 0] == 0), name
        out[name] = float(np.max(np.where(size > 0, err / np.where(size > 0, size, 1.0), 0.0)))
    return out


def capacitance_tril(cov_factor, cov_diag):
    """The Cholesky factor of I + W^T D^-1 W per particle, in float64, rounded to float32."""
    W, d = np.asarray(cov_factor, np.float64), np.asarray(cov_diag, np.float64)
    C = np.eye(W.shape[-1]) + np.einsum("kjr,kj,kjs->krs", W, 1.0 / d, W)
    return np.linalg.cholesky(C).astype(np.float32)


# ---- the kernel tests' inputs ------------------------------------------------------------------
KERNEL_DR = ((1, 1), (3, 2), (33, 31), (32, 32), (65, 33), (130, 64), (40, 128))
KERNEL_N = (1, 5, 65)
KERNEL_K = (1, 3)
# which parameters the particles share (stride 0), and whether they share the value
SHARED = ((), ("loc",), ("cov_factor",), ("cov_diag",), ("loc", "cov_factor", "cov_diag"))
PARAMS = ("loc", "cov_factor", "cov_diag")


def kernel_case(D, R, N, K, shared=(), value_shared=False):
    """float32 inputs seeded by the shape: W ~ N(0, 1), d ~ U[0.3, 2], loc ~ 3 N(0, 1), x drawn from
    the model, L from :func:`capacitance_tril` and a non-uniform upstream g ~ N(0, 1). A shared
    array has a leading axis of 1."""
    rng = np.random.default_rng([D, R, N, K, SHARED.index(tuple(shared)), int(value_shared)])
    lead = {name: 1 if name in shared else K for name in PARAMS}
    loc = (3.0 * rng.normal(0.0, 1.0, (lead["loc"], D))).astype(np.float32)
    W = rng.normal(0.0, 1.0, (lead["cov_factor"], D, R)).astype(np.float32)
    d = rng.uniform(0.3, 2.0, (lead["cov_diag"], D)).astype(np.float32)
    Kv = 1 if value_shared else K
    x = loc[:Kv, None, :].astype(np.float64) + \
        np.einsum("kjr,kir->kij", W[:Kv].astype(np.float64), rng.normal(size=(Kv, N, R))) + \
        np.sqrt(d[:Kv, None, :].astype(np.float64)) * rng.normal(size=(Kv, N, D))
    g = rng.normal(0.0, 1.0, (K, N)).astype(np.float32)
    return {"value": x.astype(np.float32), "loc": loc, "cov_factor": W, "cov_diag": d,
            "capacitance_tril": capacitance_tril(W, d), "g": g}


def kernel_cases(D, R):
    """Every case of one (D, R): N x K x layouts (at K = 1 the layouts coincide: dense alone)."""
    for N, K in itertools.product(KERNEL_N, KERNEL_K):
        layouts = itertools.product(SHARED, (False, True)) if K > 1 else [((), False), ((), True)]
        for shared, value_shared in layouts:
            yield (N, K, shared, value_shared), kernel_case(D, R, N, K, shared, value_shared)


def reference(case):
    return closed_form(case["value"], case["loc"], case["cov_factor"], case["cov_diag"], case["g"])


def torch_float32(value, loc, cov_factor, cov_diag, g, dtype=None):
    """torch's LowRankMultivariateNormal.log_prob and its autograd on the host, through the
    constructor, in float32 (or ``dtype``): the same dict as :func:`closed_form` (per particle)."""
    import torch
    from torch.distributions import LowRankMultivariateNormal
    dtype = dtype or torch.float32
    K = g.shape[0]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # one summation order, whatever the machine
    try:
        leaves = [torch.tensor(np.broadcast_to(a, (K,) + a.shape[1:]).copy(), dtype=dtype,
                               requires_grad=True) for a in (value, loc, cov_factor, cov_diag)]
        x, m, W, d = leaves
        dist = LowRankMultivariateNormal(m[:, None], W[:, None], d[:, None], validate_args=False)
        lp = dist.log_prob(x)
        grads = torch.autograd.grad((torch.tensor(np.asarray(g), dtype=dtype) * lp).sum(), leaves)
    finally:
        torch.set_num_threads(threads)
    out = {"log_prob": lp.detach().numpy()}
    out.update({name: t.numpy() for name, t in zip(GRADS, grads)})
    return out


# torch_float32's largest fraction of each quantity over every case of kernel_cases(D, R), (D, R) in
# KERNEL_DR (tests/test_lowrank_site_host.py recomputes them): what the kernels' bounds are 4 x of.
TORCH_F32 = {
    "log_prob": 3.03e-7,
    "dvalue": 1.67e-6,
    "dloc": 8.68e-7,
    "dcov_factor": 1.38e-4,
    "dcov_diag": 4.44e-7,
}
