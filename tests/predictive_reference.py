"""
NumPy restatement of the predictive draws (csrc/predictive.hip, include/mininf_amd.h
mi_predictive_*) from raw Philox words, for tests/test_gpu_predictive_families.py; checked against
itself in tests/test_predictive_host.py.

The words come from the oracle's plain-C generator (``oracle_philox4x32`` of oracle/liboracle.so,
7 rounds, the guide generator). ``u01`` is restated exactly in float32. Every draw takes
``dtype``: with ``np.float64`` (the reference) all arithmetic after ``u01`` is float64; with
``np.float32`` it is float32 in the kernels' order and each transcendental is the correctly
rounded float32 value, which is what distinguishes a formula that tolerates float32 from one that
does not. The parts the kernels themselves evaluate in float64 (Poisson's transformed rejection)
are float64 under both.

Draws that decide by a comparison also return ``marked``: True where the compared quantities lie
within the stated band of each other, so that float32 rounding may decide the other way.
"""
import ctypes
import functools

import numpy as np
import torch

from oracle import build as oracle_build

GUIDE_ROUNDS = 7
# u is clamped below 1 where u = 1 would be a pole (Laplace, Cauchy, HalfCauchy): the top grid
# point (2^24 - 1/2) 2^-24 rounds to 1.0f
BELOW_ONE = np.float32(1.0 - 2.0 ** -24)


@functools.lru_cache(maxsize=None)
def _philox():
    handle = ctypes.CDLL(oracle_build.build())
    fn = handle.oracle_philox4x32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                   ctypes.c_void_p]
    fn.restype = None
    return fn


def philox(counters: np.ndarray, seed: int) -> np.ndarray:
    """Philox-4x32-7 blocks [n, 4] (uint32) of the counters [n, 4] under key = seed."""
    ctr = np.ascontiguousarray(counters, dtype=np.uint32)
    out = np.empty_like(ctr)
    fn, k0, k1 = _philox(), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    src, dst = ctr.ctypes.data, out.ctypes.data
    for i in range(ctr.shape[0]):
        fn(src + 16 * i, k0, k1, GUIDE_ROUNDS, dst + 16 * i)
    return out


def u01(bits: np.ndarray) -> np.ndarray:
    """((bits >> 8) + 1/2) 2^-24 rounded once to float32 (device_math.hpp u01)."""
    return (((bits >> 8).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)


@functools.lru_cache(maxsize=64)
def quad_words(seed: int, stream_id: int, n: int) -> np.ndarray:
    """Words of elements 0 .. n-1 of the fixed-consumption stream: element e is word e % 4 of
    counter {e / 4, 0, 0, stream_id << 8} (guide_bits at step 0, sub-stream 0, particle 0)."""
    quads = (n + 3) // 4
    ctr = np.zeros((quads, 4), np.uint32)
    ctr[:, 0] = np.arange(quads, dtype=np.uint64).astype(np.uint32)
    ctr[:, 3] = (stream_id << 8) & 0xFFFFFFFF
    words = philox(ctr, seed).reshape(-1)[:n]
    words.setflags(write=False)
    return words


def uniforms(seed: int, stream_id: int, n: int) -> np.ndarray:
    return u01(quad_words(seed, stream_id, n))


def _f(fn, x, dtype):
    """fn(x) in float64, rounded to dtype."""
    return fn(np.asarray(x, np.float64)).astype(dtype)


def normals(seed: int, stream_id: int, n: int, dtype=np.float64) -> np.ndarray:
    """Box-Muller of device_math.hpp: words (0, 1) of a quad give elements 0 and 1, words (2, 3)
    elements 2 and 3; r = sqrt(-2 log u_a), (r cos 2 pi u_b, r sin 2 pi u_b)."""
    padded = 4 * ((n + 3) // 4)
    u = uniforms(seed, stream_id, padded).reshape(-1, 2)
    ua, ub = u[:, 0].astype(dtype), u[:, 1].astype(dtype)
    r = _f(np.sqrt, dtype(-2.0) * _f(np.log, ua, dtype), dtype)
    t = np.asarray(ub, np.float64) * (2.0 * np.pi)
    out = np.stack([r * np.cos(t).astype(dtype), r * np.sin(t).astype(dtype)], axis=1)
    return out.reshape(-1)[:n].astype(dtype)


# ---- fixed-consumption families: parameters and noise are arrays of one shape ------------------
def bernoulli_probs(p, u):
    """Exact: the same float32 comparison as the kernel's."""
    return (np.asarray(u, np.float32) < np.asarray(p, np.float32)).astype(np.float64)


def bernoulli_logits(logits, u, dtype=np.float64):
    l = np.asarray(logits, dtype)
    p = dtype(1.0) / (dtype(1.0) + _f(np.exp, -l, dtype))
    u = np.asarray(u, dtype)
    marked = np.abs(u.astype(np.float64) - p.astype(np.float64)) < 1e-6
    return (u < p).astype(np.float64), marked


def exponential(rate, u, dtype=np.float64):
    return (-_f(np.log, np.asarray(u, dtype), dtype) / np.asarray(rate, dtype)).astype(np.float64)


def laplace(loc, scale, u, dtype=np.float64):
    d = np.minimum(np.asarray(u, np.float32), BELOW_ONE).astype(dtype) - dtype(0.5)
    tail = _f(np.log1p, dtype(-2.0) * np.abs(d), dtype)
    out = np.asarray(loc, dtype) - np.asarray(scale, dtype) * np.sign(d) * tail
    return out.astype(np.float64)


def _tan_half_turns(x, dtype):
    """tan(pi x) as sin(pi x) / cos(pi x) of the exact x (the kernel's sincospif)."""
    x = np.asarray(x, np.float64)
    return _f(np.sin, np.pi * x, dtype) / _f(np.cos, np.pi * x, dtype)


def cauchy(loc, scale, u, dtype=np.float64):
    d = np.minimum(np.asarray(u, np.float32), BELOW_ONE).astype(dtype) - dtype(0.5)
    out = np.asarray(loc, dtype) + np.asarray(scale, dtype) * _tan_half_turns(d, dtype)
    return out.astype(np.float64)


def half_cauchy(scale, u, dtype=np.float64):
    h = dtype(0.5) * np.minimum(np.asarray(u, np.float32), BELOW_ONE).astype(dtype)
    return (np.asarray(scale, dtype) * _tan_half_turns(h, dtype)).astype(np.float64)


def tangent_compared(u):
    """Where the two tangents are compared: |u - 1/2| < 1/2 - 2^-10."""
    return np.abs(np.asarray(u, np.float64) - 0.5) < 0.5 - 2.0 ** -10


def half_normal(scale, eps, dtype=np.float64):
    return (np.asarray(scale, dtype) * np.abs(np.asarray(eps, dtype))).astype(np.float64)


def log_normal(loc, scale, eps, dtype=np.float64):
    arg = np.asarray(loc, dtype) + np.asarray(eps, dtype) * np.asarray(scale, dtype)
    return _f(np.exp, arg, dtype).astype(np.float64)


# ---- Categorical -------------------------------------------------------------------------------
def categorical(logits, u, dtype=np.float64):
    """
    Rows ``logits [R, C]`` (float32) and their uniforms ``u [R]``: the smallest c with
    cum_c > u cum_{C-1}, cum_c = sum_{j <= c} exp(l_j - max l) ascending; past the end, the last
    category with a finite logit. ``marked``: |u total - cum_c| < 1e-5 total for some c.
    """
    l = np.asarray(logits, np.float32)
    R, C = l.shape
    with np.errstate(invalid="ignore"):
        e = _f(np.exp, l.astype(np.float64) - l.max(axis=1, keepdims=True).astype(np.float64),
               dtype)
    cum = np.add.accumulate(e, axis=1, dtype=dtype)
    total = cum[:, -1]
    threshold = np.asarray(u, dtype) * total
    above = cum > threshold[:, None]
    found = np.where(above.any(axis=1), above.argmax(axis=1), -1)
    finite = np.isfinite(l)
    last = np.where(finite.any(axis=1), C - 1 - finite[:, ::-1].argmax(axis=1), C - 1)
    value = np.where(found >= 0, found, last).astype(np.int64)
    gap = np.abs(threshold.astype(np.float64)[:, None] - cum.astype(np.float64))
    marked = (gap < 1e-5 * total.astype(np.float64)[:, None]).any(axis=1)
    return value, marked


def categorical_rows(logits, T):
    """logits [S, B, C] -> the [S * T * B, C] rows in draw order r = (s T + t) B + b."""
    l = np.asarray(logits, np.float32)
    S, B, C = l.shape
    return np.broadcast_to(l[:, None], (S, T, B, C)).reshape(S * T * B, C)


# ---- Poisson -----------------------------------------------------------------------------------
class _Stream:
    """gamma_sample.hpp Stream for many elements at once: blocks of counter
    {e, 0, 0, (stream_id << 8) | (sub << 6) | (block & 63)}, four words each."""
    def __init__(self, elements, seed, stream_id, sub):
        self.elements = np.asarray(elements, np.uint64)
        self.seed, self.head = seed, ((stream_id << 8) | (sub << 6)) & 0xFFFFFFFF
        n = len(self.elements)
        self.block = np.zeros(n, np.uint32)
        self.used = np.full(n, 4, np.int64)
        self.bits = np.zeros((n, 4), np.uint32)

    def uniform(self, idx):
        need = idx[self.used[idx] == 4]
        if len(need):
            ctr = np.zeros((len(need), 4), np.uint32)
            ctr[:, 0] = self.elements[need].astype(np.uint32)
            ctr[:, 3] = self.head | (self.block[need] & 63)
            self.bits[need] = philox(ctr, self.seed)
            self.block[need] += 1
            self.used[need] = 0
        words = self.bits[idx, self.used[idx]]
        self.used[idx] += 1
        return u01(words)


POISSON_FACTORS, POISSON_ATTEMPTS = 250, 64


def _near(x, bound, rel=1e-5):
    return np.abs(np.asarray(x, np.float64) - bound) < rel * np.abs(bound)


def poisson(rate, seed, stream_id, dtype=np.float64):
    """
    Poisson(rate[e]) for flat elements e = 0 .. N-1 (sub-stream 3). rate < 10: the number of
    further uniforms multiplied in before the product falls below exp(-rate). rate >= 10:
    Hoermann's PTRS (1993), float64. ``marked``: a compared quantity within 1e-5 relative of its
    bound. Also returns the Philox blocks each draw consumed.
    """
    rate = np.asarray(rate, np.float32).reshape(-1)
    N = len(rate)
    rng = _Stream(np.arange(N), seed, stream_id, 3)
    value = np.zeros(N, np.float64)
    marked = np.zeros(N, bool)
    with np.errstate(invalid="ignore"):
        invalid = ~(rate >= 0) | ~np.isfinite(rate)
    value[invalid] = np.nan
    valid = ~invalid

    idx = np.flatnonzero(valid & (rate > 0) & (rate < 10))
    if len(idx):
        limit = _f(np.exp, -rate[idx].astype(np.float64), dtype)
        p = rng.uniform(idx).astype(dtype)
        k = np.zeros(len(idx), np.int64)
        active = np.ones(len(idx), bool)
        for _ in range(POISSON_FACTORS):
            marked[idx[active & _near(p, limit.astype(np.float64))]] = True
            active = active & (p >= limit)
            if not active.any():
                break
            k[active] += 1
            p[active] = p[active] * rng.uniform(idx[active]).astype(dtype)
        value[idx] = k

    idx = np.flatnonzero(valid & (rate >= 10))
    if len(idx):
        lam = rate[idx].astype(np.float64)
        slam, loglam = np.sqrt(lam), np.log(lam)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        result = np.floor(lam)
        active = np.ones(len(idx), bool)
        for _ in range(POISSON_ATTEMPTS):
            w = np.flatnonzero(active)
            if not len(w):
                break
            U = rng.uniform(idx[w]).astype(np.float64) - 0.5
            V = rng.uniform(idx[w]).astype(np.float64)
            us = 0.5 - np.abs(U)
            with np.errstate(divide="ignore", invalid="ignore"):
                k = np.floor((2.0 * a[w] / us + b[w]) * U + lam[w] + 0.43)
                first = (us >= 0.07) & (V <= vr[w])
                reject = ~first & ((k < 0) | ((us < 0.013) & (V > us)))
                test = ~first & ~reject
                lhs = np.log(V) + np.log(invalpha[w]) - np.log(a[w] / (us * us) + b[w])
                kk = np.where(test, k, 0.0)
                rhs = -lam[w] + kk * loglam[w] - torch.lgamma(torch.from_numpy(kk + 1.0)).numpy()
                second = test & (lhs <= rhs)
                close = _near(us, 0.07) | _near(V, vr[w]) | \
                    (~first & (_near(us, 0.013) | ((us < 0.0131) & _near(V, us)))) | \
                    (test & _near(lhs, rhs))
            marked[idx[w[close]]] = True
            done = first | second
            result[w[done]] = k[done]
            active[w[done]] = False
        value[idx] = result
    return value, marked, rng.block.astype(np.int64)


# ---- the inputs of the GPU tests (shared with the host self-consistency test) -------------------
SEED = 0x2F6E2B1C59D3A7
# the stream of the fixed-consumption cases: over SHAPES x LAYOUTS, 0.15 % of its uniforms fall in
# the band next to the tangents' poles that is left out of their comparison (the band holds
# 2 * 2^-10 = 0.2 % of a uniform's mass; tests/test_predictive_host.py asserts the share)
FIXED_STREAM = 10
SHAPES = [(S, M) for S in (1, 5, 33) for M in (1, 3, 4, 5, 257)]
LAYOUTS = ("sample", "element", "dense")   # per-sample scalar, per-element constant, dense
# family -> ((low, high) of each parameter); LogNormal keeps |loc + eps scale| < 2 (|eps| <= 5.89),
# where float32 rounds the exponent's argument to 6e-8, inside the 2e-7 of its eps identity
FIXED = {
    "bernoulli_probs": ((0.0, 1.0),),
    "bernoulli_logits": ((-6.0, 6.0),),
    "exponential": ((0.1, 5.0),),
    "laplace": ((-2.0, 2.0), (0.1, 3.0)),
    "cauchy": ((-2.0, 2.0), (0.1, 3.0)),
    "half_cauchy": ((0.1, 3.0),),
    "half_normal": ((0.1, 3.0),),
    "log_normal": ((-0.5, 0.5), (0.05, 0.25)),
}
PROB_CORNERS = np.array([0.0, 1.0, 2.0 ** -25, 1.0 - 2.0 ** -24], np.float32)


def fixed_parameters(family, S, M, layout):
    """float32 parameters of one case, shaped [S, 1], [1, M] or [S, M]."""
    shape = {"sample": (S, 1), "element": (1, M), "dense": (S, M)}[layout]
    rng = np.random.default_rng([S, M, LAYOUTS.index(layout), sorted(FIXED).index(family)])
    params = [rng.uniform(low, high, shape).astype(np.float32) for low, high in FIXED[family]]
    if family == "bernoulli_probs":
        flat = params[0].reshape(-1)
        flat[:len(PROB_CORNERS)] = PROB_CORNERS[:len(flat)]
    return params


def fixed_draw(family, params, seed, stream_id, S, M, dtype=np.float64):
    """(values [S, M] float64, marked or None, u [S, M]) of one fixed-consumption case."""
    u = uniforms(seed, stream_id, S * M).reshape(S, M)
    marked = None
    if family in ("half_normal", "log_normal"):
        eps = normals(seed, stream_id, S * M, dtype).reshape(S, M)
        value = globals()[family](*params, eps, dtype)
    elif family == "bernoulli_probs":
        value = bernoulli_probs(np.broadcast_to(params[0], (S, M)), u)
    elif family == "bernoulli_logits":
        value, marked = bernoulli_logits(np.broadcast_to(params[0], (S, M)), u, dtype)
    else:
        value = globals()[family](*params, u, dtype)
    return np.broadcast_to(value, (S, M)), marked, u


def relative_error(family, params, got, want):
    """|got - want| over the size of the draw's terms: |loc| + |want - loc| for the location
    families (float32 rounds their sum relative to the larger term, and loc + scale t crosses
    zero), |want| for the others."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    size = np.abs(want)
    if family in ("laplace", "cauchy"):
        loc = np.asarray(params[0], np.float64)
        size = np.abs(loc) + np.abs(want - loc)
    return np.abs(got - want) / size


CATEGORICAL_CASES = [(C, B, T) for C in (1, 2, 3, 32, 33, 37, 130) for B in (1, 3) for T in (1, 4)]
CATEGORICAL_S = 33


def categorical_logits(C, B, layout="dense"):
    """logits [S, B, C] (or [1, B, C] for "element"): random rows, then one row whose trailing
    categories are -inf and one with all its mass on one category."""
    S = 1 if layout == "element" else CATEGORICAL_S
    rng = np.random.default_rng([C, B, LAYOUTS.index(layout)])
    l = rng.normal(0.0, 2.0, (S, B, C)).astype(np.float32)
    l[0, 0, C // 2 + 1:] = -np.inf
    if S > 1:
        l[1, B - 1, :] = -np.inf
        l[1, B - 1, C // 3] = 0.5
    return l


POISSON_RATES = np.array([0.0, 0.05, 0.7, 3.0, 9.99, 10.0, 37.5, 1000.0, 1e6], np.float32)
POISSON_SHAPE = (33, 606)   # S * M = 19998: each rate about 2222 times


def poisson_rates():
    S, M = POISSON_SHAPE
    return POISSON_RATES[np.arange(S * M) % len(POISSON_RATES)].reshape(S, M)
