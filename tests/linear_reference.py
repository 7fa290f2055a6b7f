"""
The fp64 reference, the launch helper and the launch geometry of the linear-predictor site kernels
(mi_linear_forward), shared by test_gpu_linear.py, test_gpu_linear_variants.py and
test_linear_geometry_host.py.

reference():  Normal(X @ theta, sigma) / Bernoulli(logits = X @ theta) log densities and their
              gradients in fp64 numpy (normal.py:88-103, bernoulli.py:121-125), with an optional
              row_index and an optional folded prior over theta (Normal, Beta or Gamma; fp64 with
              math.lgamma). Evaluated in chunks of at most 1024 particles.
launch():     one mi_linear_forward through the C ABI over poisoned buffers: the workspace sits
              between two 256-byte guards and is all 0xFF bytes (every float a NaN), `total` and
              `dslots` are NaN, the flag words 0xFFFFFFFF -- a partial the kernel fails to write or
              a flag word the launch fails to clear cannot pass for a value. After the launch the
              guards must be intact and, without gradients, dslots untouched.
run():        launch() with the return code checked: (total, dslots, flags).
geometry():   a Python restatement of geometry() in csrc/linear.hip, for the tests to assert the
              kernel variant a shape lands in. test_linear_geometry_host.py holds it to the
              library's mi_linear_workspace_bytes.
"""
import ctypes
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from mininf_amd import _native as nat

# A folded prior over theta: family (nat.NORMAL: loc, scale; nat.BETA: c1, c0; nat.GAMMA:
# concentration, rate), its two constants and the prior site's own scale.
Prior = namedtuple("Prior", "family c0 c1 scale")

PARTICLE_CHUNK = 1024
GUARD = 256


# ---- launch geometry (csrc/linear.hip, geometry()) ---------------------------------------------
MF_THREADS = 256          # kMfVariants: both variants run 256 threads
MF_STAGE_ROWS = 128       # rows per stage with one feature tile (MfShape::CH = 128 / PT)
MF_TARGET_BLOCKS = 1024   # blocks aimed at over the grid (divided by gy)
VALU_CHUNK = 64           # kLinChunk
VALU_TARGET_BLOCKS = 768
FIN_CHUNK = 256           # kFinChunk (csrc/reduce.hip): chunked finalize above 2 * FIN_CHUNK tiles


def ceil_div(a, b):
    return -(-a // b)


def geometry(N, P, K, per_particle_sigma, prior, mfma_eligible):
    """
    The launch of an [N rows, P features, K particles] site. per_particle_sigma: a Normal site with
    a sigma per particle (one more gradient slot); prior: a folded prior is present; mfma_eligible:
    the inputs meet the matrix-core kernel's conditions (P % 4 == 0, unit feature stride, row stride
    a multiple of 4 floats, 16-byte aligned base, MI_LINEAR_VALU not set).
    """
    g = SimpleNamespace()
    g.nv = 1 + P + (1 if per_particle_sigma else 0)
    g.mfma = bool(mfma_eligible)
    if g.mfma:
        g.pt = 1 if P <= 32 else 2
        waves = MF_THREADS // 64
        ptiles = ceil_div(K, 32)
        wt = 1
        while wt < waves and wt < ptiles:
            wt <<= 1
        g.wt = wt
        g.gy = ceil_div(ptiles, wt)
        g.stage_rows = MF_STAGE_ROWS // g.pt
        g.nstage = ceil_div(N, g.stage_rows)
        target = max(1, MF_TARGET_BLOCKS // g.gy)
        g.stages_per_block = ceil_div(g.nstage, target)
        row_blocks = ceil_div(g.nstage, g.stages_per_block)
        g.gx = ceil_div(row_blocks, 8) * 8
        g.row_subsets = waves // wt
        items = 16 * g.pt + 2
        g.lds_floats = g.stage_rows * (32 * g.pt + 4)
        g.combine_floats = (g.row_subsets - 1) * wt * 64 * items
        g.combine = g.row_subsets > 1 and g.combine_floats <= g.lds_floats
        g.ntile = (g.gx if g.combine else g.gx * g.row_subsets) + (1 if prior else 0)
        g.empty_row_blocks = g.gx - row_blocks
        g.last_block_stages = g.nstage - (row_blocks - 1) * g.stages_per_block
        g.last_stage_rows = N - (g.nstage - 1) * g.stage_rows
    else:
        g.pt = g.wt = 0
        kb = 1
        while kb < 256 and kb < K:
            kb <<= 1
        g.kb = kb
        g.gy = ceil_div(K, kb)
        tiles = max(1, VALU_TARGET_BLOCKS // g.gy)
        g.rows_per_tile = max(VALU_CHUNK, ceil_div(ceil_div(N, tiles), VALU_CHUNK) * VALU_CHUNK)
        g.ntile = ceil_div(N, g.rows_per_tile)
        g.gx = g.ntile
        g.stages_per_block = 0
        g.combine = False
        g.empty_row_blocks = 0
        g.last_stage_rows = N - (ceil_div(N, VALU_CHUNK) - 1) * VALU_CHUNK
    g.chunked_finalize = g.ntile > 2 * FIN_CHUNK
    g.workspace_bytes = ceil_div(g.nv * g.ntile * K * 4, 256) * 256
    if g.chunked_finalize:
        g.workspace_bytes += g.nv * ceil_div(g.ntile, FIN_CHUNK) * K * 8
    return g


def mfma_eligible(P, x_stride_i, x_stride_j, x_ptr, valu=False):
    """use_mfma() of csrc/linear.hip."""
    return (not valu and P % 4 == 0 and x_stride_j == 1 and x_stride_i >= P and
            x_stride_i % 4 == 0 and x_ptr % 16 == 0)


# ---- fp64 reference ----------------------------------------------------------------------------
def prior_terms(prior, th):
    """log p(theta) and d log p / d theta of the folded prior, elementwise in fp64."""
    a, b = float(prior.c0), float(prior.c1)
    if prior.family == nat.NORMAL:
        lp = -(th - a) ** 2 / (2 * b ** 2) - math.log(b) - 0.5 * math.log(2 * math.pi)
        d = -(th - a) / b ** 2
    elif prior.family == nat.BETA:
        lp = (a - 1) * np.log(th) + (b - 1) * np.log1p(-th) + \
            math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b)
        d = (a - 1) / th - (b - 1) / (1 - th)
    elif prior.family == nat.GAMMA:
        lp = a * math.log(b) + (a - 1) * np.log(th) - b * th - math.lgamma(a)
        d = (a - 1) / th - b
    else:
        raise ValueError(prior.family)
    return lp, d


def reference(family, X, theta, y, mask, sigma, site_scale, g0, row_index=None, prior=None):
    """
    (total [K], dtheta [K, P], dsigma [K], bound [K, P], sbound [K]): bound and sbound are the sums
    of the absolute values of the terms of dtheta / g0 and dsigma / g0.
    """
    if row_index is not None:
        X, y, mask = X[row_index], y[row_index], mask[row_index]
    X64 = X.astype(np.float64)
    absX = np.abs(X64)
    m = mask.astype(np.float64)[:, None]
    y64 = np.where(mask, y, 0.0).astype(np.float64)[:, None]   # masked lanes are never read
    K, P = theta.shape
    total, dsigma, sbound = np.empty(K), np.empty(K), np.empty(K)
    dtheta, bound = np.empty((K, P)), np.empty((K, P))
    for k0 in range(0, K, PARTICLE_CHUNK):
        k1 = min(K, k0 + PARTICLE_CHUNK)
        th = theta[k0:k1].astype(np.float64)
        mu = X64 @ th.T                                   # [N, chunk]
        if family == nat.NORMAL:
            s = sigma[k0:k1].astype(np.float64)[None, :]
            d = y64 - mu
            lp = -d ** 2 / (2 * s ** 2) - np.log(s) - 0.5 * np.log(2 * np.pi)
            dmu = d / s ** 2
            dsig = d ** 2 / s ** 3 - 1 / s
        else:
            lp = y64 * mu - np.logaddexp(0.0, mu)
            e = np.exp(-np.abs(mu))                       # sigmoid without overflow
            dmu = y64 - np.where(mu >= 0, 1 / (1 + e), e / (1 + e))
            dsig = np.zeros_like(mu)
        total[k0:k1] = site_scale * (m * lp).sum(0)
        dtheta[k0:k1] = g0 * site_scale * ((m * dmu).T @ X64)
        dsigma[k0:k1] = g0 * site_scale * (m * dsig).sum(0)
        bound[k0:k1] = site_scale * (np.abs(m * dmu).T @ absX) + 1e-6
        sbound[k0:k1] = site_scale * np.abs(m * dsig).sum(0) + 1e-6
        if prior is not None:
            plp, pd = prior_terms(prior, th)
            total[k0:k1] += prior.scale * plp.sum(1)
            dtheta[k0:k1] += g0 * prior.scale * pd
            bound[k0:k1] += np.abs(prior.scale * pd)
    return total, dtheta, dsigma, bound, sbound


# ---- launch ------------------------------------------------------------------------------------
Result = namedtuple("Result", "rc total dslots flags prior_flags geometry")


def launch(family, X, theta, y, mask, sigma, sigma_per_particle, site_scale, g0, valu,
           compute_grads=1, row_index=None, prior=None, flags_zeroed=False):
    """
    One mi_linear_forward over poisoned buffers. X, theta, y, mask, sigma and row_index (int32) are
    device tensors and may be strided views: their strides go to the site as they are. Returns
    Result(rc, total [K], dslots [slots, K], flags, prior_flags, geometry) without raising on rc.
    """
    import torch
    device = X.device
    P = X.shape[1]
    N = X.shape[0] if row_index is None else row_index.shape[0]
    K = theta.shape[0]
    L = nat.Linear()
    L.K, L.N, L.P = K, N, P
    L.family = family
    L.options = (nat.LINEAR_VALU if valu else 0) | (nat.GROUP_FLAGS_ZEROED if flags_zeroed else 0)
    L.x = X.data_ptr()
    L.x_stride_i, L.x_stride_j = X.stride()
    L.theta = theta.data_ptr()
    L.theta_stride_k, L.theta_stride_j = theta.stride()
    L.value = y.data_ptr()
    L.value_stride_i = y.stride(0)
    if mask is not None:
        L.mask = mask.data_ptr()
        L.mask_stride_i = mask.stride(0)
    if sigma_per_particle:
        L.scale = sigma.data_ptr()
        L.scale_stride_k = sigma.stride(0)
    else:
        L.scale_constant = float(sigma[0])
    L.grad_scale = g0
    L.site_scale = site_scale
    L.compute_grads = compute_grads
    if row_index is not None:
        assert row_index.dtype == torch.int32 and row_index.is_contiguous()
        L.row_index = row_index.data_ptr()
    poison = 0 if flags_zeroed else -1    # 0xFFFFFFFF
    flags = torch.full((1,), poison, dtype=torch.int32, device=device)
    prior_flags = torch.full((1,), poison, dtype=torch.int32, device=device)
    if prior is not None:
        L.prior.present = 1
        L.prior.family = prior.family
        L.prior.constant[0], L.prior.constant[1] = prior.c0, prior.c1
        L.prior.scale = prior.scale
        L.prior.flags = prior_flags.data_ptr()
    per_particle = bool(sigma_per_particle) and family == nat.NORMAL
    geo = geometry(N, P, K, per_particle, prior is not None,
                   mfma_eligible(P, L.x_stride_i, L.x_stride_j, L.x, valu))
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "workspace")
    assert size.value == geo.workspace_bytes, (size.value, vars(geo))
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    total = torch.full((K,), float("nan"), device=device)
    nslots = P + (1 if sigma_per_particle else 0)
    dslots = torch.full((nslots, K), float("nan"), device=device)
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


def run(family, X, theta, y, mask, sigma, sigma_per_particle, site_scale, g0, valu, **options):
    """launch() that raises on a failed return code: (total, dslots, flags)."""
    r = launch(family, X, theta, y, mask, sigma, sigma_per_particle, site_scale, g0, valu,
               **options)
    nat.check(r.rc, "mi_linear_forward")
    return r.total, r.dslots, r.flags
