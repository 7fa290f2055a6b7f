"""
NumPy float64 restatement of the Normal-mixture site (csrc/mixture.hip, include/mininf_amd.h
mi_mixture_normal_forward) and of its predictive draw (mi_predictive_mixture_normal), with the
inputs tests/test_gpu_mixture.py and tests/test_mixture_host.py share.

The draw is restated from ``tests.predictive_reference.philox``: the component is
``predictive_reference.categorical`` on the uniforms of sub-stream 0, eps the Box-Muller output of
sub-stream 1 (the counter's last word is ``(stream_id << 8) | sub``).
"""
import functools

import numpy as np

from tests import predictive_reference as ref

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


# ---- the site ----------------------------------------------------------------------------------
def closed_form(logits, loc, scale, x, mask=None, batch_scale=1.0, g0=1.0):
    """
    The site in float64 for inputs broadcastable to logits/loc/scale [K, N, C], x [K, N],
    mask [N]. Returns a dict: ``total`` [K], ``dlogits``/``dloc``/``dscale`` [K, N, C], ``dvalue``
    [K, N] (g0 * batch_scale folded in, zeros on masked rows), ``row`` [K, N] the rows' log
    densities, ``r`` the responsibilities, and the sizes the error bounds are relative to:
    ``total_size`` [K] = batch_scale * sum_i mask_i (max_c |t_ic| + 1) and ``*_size`` = |g0 *
    batch_scale| times the sum of the absolute terms of each gradient's formula.
    """
    logits, loc, scale, x = (np.asarray(a, np.float64) for a in (logits, loc, scale, x))
    shape = np.broadcast_shapes(logits.shape, loc.shape, scale.shape, x.shape + (1,))
    logits, loc, scale = (np.broadcast_to(a, shape) for a in (logits, loc, scale))
    x = np.broadcast_to(x, shape[:-1])
    on = np.ones(shape[1], bool) if mask is None else np.asarray(mask, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lmax = logits.max(-1, keepdims=True)
        m = logits - (lmax + np.log(np.exp(logits - lmax).sum(-1, keepdims=True)))
        z = (x[..., None] - loc) / scale
        t = m - np.log(scale) - HALF_LOG_2PI - 0.5 * z * z
        tmax = t.max(-1, keepdims=True)
        row = (tmax + np.log(np.exp(t - tmax).sum(-1, keepdims=True)))[..., 0]
        r = np.exp(t - row[..., None])
        pm = np.exp(m)
        finite_t = np.where(np.isfinite(t), np.abs(t), 0.0)
    g = g0 * batch_scale
    on3 = on[None, :, None]
    rz = r * z / scale
    out = {
        "row": row, "r": r, "t": t,
        "total": batch_scale * np.where(on[None], row, 0.0).sum(1),
        "total_size": abs(batch_scale) * np.where(on[None], finite_t.max(-1) + 1.0, 0.0).sum(1),
        "dlogits": np.where(on3, g * (r - pm), 0.0),
        "dlogits_size": abs(g) * (r + pm),
        "dloc": np.where(on3, g * rz, 0.0),
        "dloc_size": abs(g) * np.abs(rz),
        "dscale": np.where(on3, g * r * (z * z - 1.0) / scale, 0.0),
        "dscale_size": abs(g) * (r * z * z / scale + r / scale),
        "dvalue": np.where(on[None], -g * rz.sum(-1), 0.0),
        "dvalue_size": abs(g) * np.abs(rz).sum(-1),
    }
    return out


GRADS = ("dlogits", "dloc", "dscale", "dvalue")


# dloc and dscale are single products with r_c: where float64 holds an r_c that float32 cannot
# (below 2^-126, or 2^-149 with denormals) the float32 entry is 0 and its error is all of its
# size. The "_clear" fractions are taken over the entries whose r_c is at least this, far from
# float32's underflow.
CLEAR_R = 2.0 ** -64


def fractions(got, want):
    """Largest error of ``got`` (a dict with total and the four gradients) over its size in
    ``want``: {"total": .., "dlogits": .., ...}, and "dloc_clear" / "dscale_clear" over the entries
    with r_c >= CLEAR_R alone. Entries of size 0 must be exact zeros."""
    out = {}
    for name in ("total",) + GRADS:
        if got.get(name) is None:
            continue
        g, w, size = np.asarray(got[name], np.float64), want[name], want[name + "_size"]
        assert not np.isnan(g).any(), name
        err = np.abs(g - w)
        assert np.all(err[size == 0] == 0), name
        frac = np.where(size > 0, err / np.where(size > 0, size, 1.0), 0.0)
        out[name] = float(np.max(frac))
        if name in ("dloc", "dscale"):
            out[name + "_clear"] = float(np.max(np.where(want["r"] >= CLEAR_R, frac, 0.0)))
    return out


# ---- the kernel tests' inputs ------------------------------------------------------------------
KERNEL_C = (1, 2, 3, 31, 32, 33, 64, 65, 257, 1024)
KERNEL_N = (1, 5)
KERNEL_K = (1, 7, 64)
LAYOUTS = ("dense", "particle_constant", "row_constant")


def kernel_case(C, N, K, layout="dense"):
    """float32 (logits, loc, scale) shaped [K, N, C] -- [1, N, C] when particle-constant,
    [K, 1, C] when row-constant -- and x [K, N] drawn from the mixture: logits N(0, 1), locs
    3 N(0, 1), scales U[0.3, 2]."""
    rng = np.random.default_rng([C, N, K, LAYOUTS.index(layout)])
    shape = {"dense": (K, N, C), "particle_constant": (1, N, C), "row_constant": (K, 1, C)}[layout]
    logits = rng.normal(0.0, 1.0, shape).astype(np.float32)
    loc = (3.0 * rng.normal(0.0, 1.0, shape)).astype(np.float32)
    scale = rng.uniform(0.3, 2.0, shape).astype(np.float32)
    full = (K, N, C)
    p = np.exp(np.broadcast_to(logits, full).astype(np.float64))
    cum = np.cumsum(p / p.sum(-1, keepdims=True), -1)
    comp = np.minimum((rng.random((K, N, 1)) > cum).sum(-1), C - 1)[..., None]
    mu = np.take_along_axis(np.broadcast_to(loc, full), comp, -1)[..., 0]
    sd = np.take_along_axis(np.broadcast_to(scale, full), comp, -1)[..., 0]
    x = (mu + sd * rng.normal(0.0, 1.0, (K, N))).astype(np.float32)
    return logits, loc, scale, x


def far_case():
    """One row 40 standard deviations (of the widest component) beyond every component."""
    logits, loc, scale, x = kernel_case(5, 3, 2)
    x = x.copy()
    x[:, 1] = (loc[:, 1] + 40.0 * scale[:, 1]).max(-1) + 40.0 * scale[:, 1].max(-1)
    return logits, loc, scale, x


def torch_float32(logits, loc, scale, x, mask=None, batch_scale=1.0, g0=1.0, dtype=None):
    """torch's MixtureSameFamily.log_prob and its autograd on the host, in float32 (or ``dtype``):
    the same dict of total and gradients as :func:`closed_form`."""
    import torch
    from torch.distributions import Categorical, MixtureSameFamily, Normal
    dtype = dtype or torch.float32
    K, N, C = np.broadcast_shapes(logits.shape, loc.shape, scale.shape, x.shape + (1,))
    leaves = [torch.tensor(np.broadcast_to(a, (K, N, C)).copy(), dtype=dtype, requires_grad=True)
              for a in (logits, loc, scale)]
    xv = torch.tensor(np.broadcast_to(x, (K, N)).copy(), dtype=dtype, requires_grad=True)
    d = MixtureSameFamily(Categorical(logits=leaves[0]), Normal(leaves[1], leaves[2]),
                          validate_args=False)
    row = d.log_prob(xv)
    on = torch.ones(N, dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask, bool))
    total = batch_scale * torch.where(on[None], row, torch.zeros((), dtype=dtype)).sum(1)
    grads = torch.autograd.grad(g0 * total.sum(), leaves + [xv])
    out = {"total": total.detach().numpy()}
    out.update({name: g.numpy() for name, g in zip(GRADS, grads)})
    return out


# ---- the predictive draw -----------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def words(seed, stream_id, sub, n):
    """Words of elements 0 .. n-1 of sub-stream ``sub``: element e is word e % 4 of counter
    {e / 4, 0, 0, (stream_id << 8) | sub} (guide_bits at step 0, particle 0)."""
    quads = (n + 3) // 4
    ctr = np.zeros((quads, 4), np.uint32)
    ctr[:, 0] = np.arange(quads, dtype=np.uint64).astype(np.uint32)
    ctr[:, 3] = ((stream_id << 8) | (sub & 0xFF)) & 0xFFFFFFFF
    out = ref.philox(ctr, seed).reshape(-1)[:n]
    out.setflags(write=False)
    return out


def normals(seed, stream_id, sub, n, dtype=np.float64):
    """predictive_reference.normals on sub-stream ``sub``: words (0, 1) of a quad give elements 0
    and 1, words (2, 3) elements 2 and 3; r = sqrt(-2 log u_a), (r cos 2 pi u_b, r sin 2 pi u_b)."""
    padded = 4 * ((n + 3) // 4)
    u = ref.u01(words(seed, stream_id, sub, padded)).reshape(-1, 2)
    ua, ub = u[:, 0].astype(dtype), u[:, 1].astype(dtype)
    r = ref._f(np.sqrt, dtype(-2.0) * ref._f(np.log, ua, dtype), dtype)
    t = np.asarray(ub, np.float64) * (2.0 * np.pi)
    out = np.stack([r * np.cos(t).astype(dtype), r * np.sin(t).astype(dtype)], axis=1)
    return out.reshape(-1)[:n].astype(dtype)


def draw(logits, loc, scale, S, T, seed, stream_id, dtype=np.float64):
    """
    The S * T * B draws of logits / loc / scale [S, B, C] (float32; [1, B, C] for parameters the
    samples share) in row order r = (s T + t) B + b: (value float64, component, marked, size) with
    ``marked`` predictive_reference.categorical's (the uniform within rounding of a cumulative
    boundary) and ``size`` = |loc_c| + |scale_c eps| of the chosen component.
    """
    B, C = logits.shape[1], logits.shape[2]
    rows = [ref.categorical_rows(np.broadcast_to(a, (S, B, C)), T) for a in (logits, loc, scale)]
    R = S * T * B
    u = ref.u01(words(seed, stream_id, 0, R))
    comp, marked = ref.categorical(rows[0], u, dtype)
    eps = normals(seed, stream_id, 1, R, dtype)
    mu = np.take_along_axis(rows[1], comp[:, None], 1)[:, 0].astype(dtype)
    sd = np.take_along_axis(rows[2], comp[:, None], 1)[:, 0].astype(dtype)
    value = (mu + sd * eps).astype(np.float64)
    size = np.abs(mu.astype(np.float64)) + np.abs(sd.astype(np.float64) * eps.astype(np.float64))
    return value, comp, marked, size


# (chosen so that few draws lie within predictive_reference.categorical's band of a cumulative
# boundary: of the 1560 draws of one component count -- every shape below, parameters dense and
# shared -- at most 2, 0.13 %; tests/test_mixture_host.py asserts at most 0.25 %)
DRAW_SEED = 0x51C0FFEE1D2B43
DRAW_STREAM = 0x50003
DRAW_C = (1, 2, 3, 32, 33, 130)
DRAW_CASES = [(S, T, B, C) for S in (1, 5, 33) for T in (1, 4) for B in (1, 3) for C in DRAW_C]


def draw_parameters(S, B, C, shared=False):
    """float32 logits / loc / scale [S, B, C] ([1, B, C] when the samples share them)."""
    rng = np.random.default_rng([S, B, C, int(shared)])
    shape = (1 if shared else S, B, C)
    return (rng.normal(0.0, 1.5, shape).astype(np.float32),
            (3.0 * rng.normal(0.0, 1.0, shape)).astype(np.float32),
            rng.uniform(0.3, 2.0, shape).astype(np.float32))
