"""
NumPy restatement of the one-noise-word guide factors (csrc/elementwise_guide.hip,
include/mininf_amd.h mi_elementwise_*) for tests/test_gpu_elementwise_guide.py; checked against
torch float64 in tests/test_elementwise_guide_host.py.

The noise words come from the oracle's plain-C Philox through predictive_reference.philox, at the
guide's counter {quad, particle_offset + k, step, stream_id << 8}; the transforms are
predictive_reference's float64 restatements of the same kernels' arithmetic.
"""
import functools
import math

import numpy as np

from tests import predictive_reference as pr

FAMILIES = ("exponential", "laplace", "cauchy", "half_cauchy", "half_normal", "log_normal")
# MI_PRED_* codes (include/mininf_amd.h)
CODE = {"exponential": 2, "laplace": 3, "cauchy": 4, "half_cauchy": 5, "half_normal": 6,
        "log_normal": 7}
NORMAL_BASED = ("half_normal", "log_normal")
TWO_PARAMETERS = ("laplace", "cauchy", "log_normal")
POSITIVE = ("exponential", "half_cauchy", "half_normal", "log_normal")
# Relative-error bounds of the draws: tests/test_gpu_predictive_families.py RTOL, measured there
# for this same transform and set at four times the measurement.
DRAW_RTOL = {"exponential": 9.2e-7, "laplace": 3.9e-7, "cauchy": 6.3e-7, "half_cauchy": 7.3e-7,
             "half_normal": 2.9e-6, "log_normal": 6.5e-7}

NS = (1, 3, 4, 5, 257, 1030)
KS = (1, 5, 33, 64)
SEED, STEP, STREAM, OFFSET = 0x51C0FFEE1234, 3, 2, 5
# draws within 2^-10 of a tangent's pole are left out of the comparison; at most this share of a
# case's draws may be (the expected share is 2^-9)
LEFT_OUT_CAP = 0.01


@functools.lru_cache(maxsize=None)
def words(K, N, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET):
    """Philox words [K, N] (uint32) of a factor's stream: element i of row k is word i % 4 of
    counter {i / 4, offset + k, step, stream_id << 8}."""
    quads = (N + 3) // 4
    ctr = np.zeros((K, quads, 4), np.uint32)
    ctr[:, :, 0] = np.arange(quads, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (offset + np.arange(K, dtype=np.uint32))[:, None]
    ctr[:, :, 2] = (step ^ (step >> 32)) & 0xFFFFFFFF
    ctr[:, :, 3] = (stream_id << 8) & 0xFFFFFFFF
    out = pr.philox(ctr.reshape(-1, 4), seed).reshape(K, quads * 4)[:, :N]
    out.setflags(write=False)
    return out


def uniforms(K, N, **key):
    """u01 of the words, exactly the float32 the kernels compute."""
    return pr.u01(words(K, N, **key))


def normals(K, N, **key):
    """Box-Muller of device_math.hpp in float64 (predictive_reference.normals, on this stream):
    words (0, 1) of a quad give elements 0 and 1, words (2, 3) elements 2 and 3."""
    padded = 4 * ((N + 3) // 4)
    u = pr.u01(words(K, padded, **key)).astype(np.float64).reshape(K, -1, 2)
    r = np.sqrt(-2.0 * np.log(u[..., 0]))
    t = 2.0 * np.pi * u[..., 1]
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=-1).reshape(K, padded)[:, :N]


def noise(family, K, N, **key):
    """The base noise [K, N] of a draw in float64: uniforms, or standard normals."""
    return normals(K, N, **key) if family in NORMAL_BASED else \
        uniforms(K, N, **key).astype(np.float64)


def parameters(family, N, layout="dense"):
    """float32 parameters [N] ("dense") or [1] ("scalar": read at stride 0), in
    predictive_reference.FIXED's ranges, for which DRAW_RTOL was measured."""
    rng = np.random.default_rng([N, FAMILIES.index(family), layout == "dense"])
    shape = (N,) if layout == "dense" else (1,)
    return [rng.uniform(low, high, shape).astype(np.float32) for low, high in pr.FIXED[family]]


def clamp(family, v):
    """The noise as the guide reads it: a uniform of 1.0f is 1 - 2^-24 in every uniform family
    (the predictive Exponential alone reads 1.0f as it is)."""
    if family in NORMAL_BASED:
        return np.asarray(v, np.float64)
    return np.minimum(np.asarray(v, np.float32), pr.BELOW_ONE).astype(np.float64)


def draw(family, params, v):
    """z [K, N] in float64 from the parameters ([N] or [1]) and the base noise v [K, N]."""
    v = clamp(family, v)
    return getattr(pr, family)(*[np.asarray(p, np.float64) for p in params], v, np.float64)


def factors(family, params, v):
    """(dz/da, dz/db or None), each [K, N] in float64."""
    v = clamp(family, v)
    p = [np.asarray(q, np.float64) for q in params]
    one = np.ones_like(v)
    if family == "log_normal":
        z = np.exp(p[0] + p[1] * v)
        return z, z * v
    if family == "laplace":
        d = v - 0.5
        return one, -np.sign(d) * np.log1p(-2.0 * np.abs(d))
    if family == "cauchy":
        return one, np.tan(np.pi * (v - 0.5))
    if family == "half_cauchy":
        return np.tan(0.5 * np.pi * v) * one, None
    if family == "half_normal":
        return np.abs(v) * one, None
    return np.log(v) / (p[0] * p[0]), None   # exponential: d/drate


def entropy(family, params):
    """(sum of the elements' entropies, dH/da, dH/db or None) in float64."""
    p = [np.asarray(q, np.float64) for q in params]
    if family == "log_normal":
        loc, scale = p
        return (0.5 + 0.5 * math.log(2 * math.pi) + np.log(scale) + loc).sum(), \
            np.ones_like(loc), 1.0 / scale
    if family == "laplace":
        return (1.0 + np.log(2.0 * p[1])).sum(), np.zeros_like(p[0]), 1.0 / p[1]
    if family == "cauchy":
        return np.log(4.0 * math.pi * p[1]).sum(), np.zeros_like(p[0]), 1.0 / p[1]
    if family == "half_cauchy":
        return np.log(2.0 * math.pi * p[0]).sum(), 1.0 / p[0], None
    if family == "half_normal":
        return (0.5 + 0.5 * math.log(math.pi / 2) + np.log(p[0])).sum(), 1.0 / p[0], None
    return (1.0 - np.log(p[0])).sum(), -1.0 / p[0], None


ENTROPY_NS = (1, 5, 257)
ENTROPY_SCALES = np.array([1e-3, 0.3, 1.0, 40.0], np.float32)


def entropy_parameters(family, N):
    """Scales (or rates) cycling through ENTROPY_SCALES; a loc in [-2, 2) where there is one."""
    spread = ENTROPY_SCALES[np.arange(N) % len(ENTROPY_SCALES)]
    if family in TWO_PARAMETERS:
        loc = np.random.default_rng(N).uniform(-2.0, 2.0, N).astype(np.float32)
        return [loc, spread]
    return [spread]


def torch_distribution(family, params):
    """The torch class of a family over tensor parameters (any dtype and device)."""
    from torch import distributions as D
    cls = {"exponential": D.Exponential, "laplace": D.Laplace, "cauchy": D.Cauchy,
           "half_cauchy": D.HalfCauchy, "half_normal": D.HalfNormal,
           "log_normal": D.LogNormal}[family]
    return cls(*params)
