"""
The ELBO tail's contract (include/mininf_amd.h, "ELBO tail" and "deferred finalize reductions")
restated in float64 on plain arrays, with the magnitude sums its error bounds are made of, and the
designed shapes of tests/test_gpu_elbo_tail.py. No GPU.

A case is a dict of plain data:
  K, g0 (float32), entropy_scale, terms [list of float32 [K]], buffers [list of float32],
  factors [list of factor dicts], jobs [list of job dicts]
A factor: family ("normal" | "gamma" | "beta"), n, p0 / p1 (float32 [n]; a Normal's p0 may be None),
  weight, transform (two of 0 | 1), draw (None | "sources" | "partials") and, by draw,
  sources [list of float32 [K, n]], eps [K, n] (Normal), draws [K, n] and dgrad [K, n, 2] or None
  (Beta), partial (two float32 [rows, n]). Keys the reference does not know (storage layout,
  generator words) are the launcher's.
A job: nseg, num_sites, num_slots, scale [num_sites], slot_scale, values (one per value with a
  segment block: float32 [nseg, K], or for a rank-one value a dict u [nseg], f [K], e [K]), ksum
  (float64 [num_sites, nksum], or None).

Every compared quantity comes back as a Q: its float64 value, the magnitude sums of its
fp32-evaluated terms per family (scaled as the term enters), the sum of the absolute values of its
fp64 summands, and an extra absolute allowance.
"""
from __future__ import annotations

import collections
import math

import numpy as np
from scipy import special

f32 = np.float32
EPS32 = 2.0 ** -24   # half an ulp of float32, relative
ORDER = 1e-12        # the order of an fp64 sum, relative to the sum of absolute summands

CONCENTRATIONS = (1e-3, 0.05, 0.3, 0.999, 1.0, 1.001, 1.4616321, 2.0, 2.5, 5.999, 6.0, 12.0, 100.0,
                  1e4)
BETA_PAIRS = ((0.05, 0.05), (0.3, 12.0), (1.0, 1.0), (1e4, 1e4), (1e-3, 2.5), (0.999, 1.001),
              (1.4616321, 5.999), (6.0, 100.0), (2.0, 1e4), (12.0, 0.3), (2.5, 1.0), (100.0, 1e-3))
RATES = (1e-3, 0.5, 1.0, 20.0)

FAMILIES = ("normal", "gamma", "beta")

# ---- designed shapes (their plan branches are asserted in tests/test_elbo_reference_host.py) ----
# Normal entropy: n -> lead blocks of the forward (with K <= 8192)
NORMAL_N = {1: 1, 3: 1, 4: 1, 5: 1, 1023: 1, 8191: 1, 8193: 2, 70001: 9}
# absorbed Normal draws from sources, (n, K) -> (tk, ti, columns, slices)
NORMAL_SOURCES = {(1, 4096): (256, 1, 1, 4),    # the completion-counter path
                  (5, 3): (32, 8, 1, 1),        # more row lanes than rows
                  (300, 8): (2, 128, 3, 1),     # the LDS tree, 3 columns
                  (1000, 3): (1, 256, 4, 1)}    # a lane per element
# fused-draw partial rows, (rows, n, gradient stride) -> (tk, ti, epl)
PARTIALS = {(2, 1024, 1): (1, 256, -2),    # quads
            (2, 1023, 1): (1, 256, 4),     # four elements per lane
            (2, 1024, 2): (1, 256, 4),     # strided gradients fall out of the quad layout
            (40, 37, 1): (16, 16, 1)}      # tree
# forward-absorbed Beta draws with precomputed factors, (n, K) -> (tk, ti, slices)
BETA_DGRAD = {(1, 17): (256, 1, 1), (3, 300): (64, 4, 1), (1, 300): (256, 1, 1), (3, 17): (64, 4, 1)}
# deferred reductions, (nseg, K) -> particles per reducing block
REDUCE = {(1, 100): 64, (2, 100): 64, (70, 100): 32, (520, 100): 16, (800, 100): 8, (70, 4096): 32}

Q = collections.namedtuple("Q", "value mag sum64 extra")


def _q(value, mag=None, sum64=0.0, extra=0.0):
    value = np.asarray(value, np.float64)
    mag = {k: np.broadcast_to(np.asarray(v, np.float64), value.shape) for k, v in (mag or {}).items()}
    return Q(value, mag, np.broadcast_to(np.asarray(sum64, np.float64), value.shape),
             np.broadcast_to(np.asarray(extra, np.float64), value.shape))


def bound(q, constants, rounding=True):
    """(i) the final rounding to float, (ii) the fp32-evaluated terms, (iii) the fp64 order, and
    the quantity's extra allowance. constants: family -> C."""
    out = ORDER * q.sum64 + q.extra
    if rounding:
        out = out + EPS32 * np.abs(q.value)
    for family, mag in q.mag.items():
        out = out + constants[family] * EPS32 * mag
    return out


def digamma_magnitude(x):
    """D(x) = sum_{j < m} 1 / (x + j) + |log(x + m)|, m the recurrence steps that take x to 6: the
    sum of the absolute values of what digammaf adds (|psi| itself vanishes at 1.4616)."""
    y = np.array(x, np.float64, ndmin=1)
    mag = np.zeros_like(y)
    for _ in range(6):
        low = y < 6.0
        mag += np.where(low, 1.0 / y, 0.0)
        y = np.where(low, y + 1.0, y)
    return (mag + np.abs(np.log(y))).reshape(np.shape(x))


def normal_entropy(scale):
    """H = 0.5 + 0.5 log(2 pi) + log(scale) (normal.py:112-113): H, magnitude, dH [.., 2] and its
    magnitude."""
    s = np.asarray(scale, np.float64)
    h = 0.5 + 0.5 * math.log(2.0 * math.pi) + np.log(s)
    d = np.stack([np.zeros_like(s), 1.0 / s], -1)
    return h, np.abs(np.log(s)), d, np.abs(d)


def gamma_entropy(a, r):
    """H = a - log(r) + lgamma(a) + (1 - a) psi(a) (gamma.py:101-107)."""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    h = a - np.log(r) + special.gammaln(a) + (1.0 - a) * special.digamma(a)
    mag = np.abs(a) + np.abs(np.log(r)) + np.abs(special.gammaln(a)) + \
        np.abs(1.0 - a) * digamma_magnitude(a)
    tri = special.polygamma(1, a)
    d = np.stack([1.0 + (1.0 - a) * tri, -1.0 / r], -1)
    dmag = np.stack([1.0 + np.abs(1.0 - a) * tri, 1.0 / r], -1)
    return h, mag, d, dmag


def beta_entropy(a, b, t=None):
    """Beta(a, b) = Dirichlet([a, b]) (dirichlet.py:122-130): lgamma(a) + lgamma(b) - lgamma(t)
    - (2 - t) psi(t) - (a - 1) psi(a) - (b - 1) psi(b); t = a + b formed in float32 (the guide's
    dtype, concentration.sum(-1)) unless given."""
    if t is None:
        t = (np.asarray(a, f32) + np.asarray(b, f32)).astype(f32)
    a, b, t = (np.asarray(v, np.float64) for v in (a, b, t))
    lg, psi, tri = special.gammaln, special.digamma, lambda v: special.polygamma(1, v)
    h = lg(a) + lg(b) - lg(t) - (2.0 - t) * psi(t) - (a - 1.0) * psi(a) - (b - 1.0) * psi(b)
    mag = np.abs(lg(a)) + np.abs(lg(b)) + np.abs(lg(t)) + np.abs(2.0 - t) * digamma_magnitude(t) + \
        np.abs(a - 1.0) * digamma_magnitude(a) + np.abs(b - 1.0) * digamma_magnitude(b)
    tt = (t - 2.0) * tri(t)
    d = np.stack([tt - (a - 1.0) * tri(a), tt - (b - 1.0) * tri(b)], -1)
    dmag = np.stack([np.abs(t - 2.0) * tri(t) + np.abs(a - 1.0) * tri(a),
                     np.abs(t - 2.0) * tri(t) + np.abs(b - 1.0) * tri(b)], -1)
    return h, mag, d, dmag


def factor_entropy(f):
    if f["family"] == "normal":
        return normal_entropy(f["p1"])
    if f["family"] == "gamma":
        return gamma_entropy(f["p0"], f["p1"])
    return beta_entropy(f["p0"], f["p1"])


def source_sum(sources, shape):
    """dz [K, n]: the float32 sum of the sources in slot order (the same IEEE operations)."""
    g = np.zeros(shape, f32)
    for s in sources:
        g = (g + np.asarray(s, f32)).astype(f32)
    return g


def draw_sums(f, K, floor=0.0, linear=False):
    """The absorbed draw's particle sums s [n, 2], the sums of their absolute summands, and the
    inline Beta path's allowance (4 * floor * sum |g factor|). linear: the sources enter one by
    one, sum_s sum_k source_s[k] factor[k] in float64 -- what a launch does that finishes a
    one-element factor in the blocks that write its source rows (the header's dz = sum_s source
    without the float32 rounding of dz)."""
    n = f["n"]
    zero = np.zeros((n, 2))
    if f.get("draw") is None:
        return zero, zero, zero
    if f["draw"] == "partials":
        p = np.stack([np.asarray(v, np.float64) for v in f["partial"]], -1)   # [rows, n, 2]
        return p.sum(0), np.abs(p).sum(0), zero
    if linear:
        dz = sum(np.asarray(x, np.float64) for x in f["sources"])
    else:
        dz = source_sum(f["sources"], (K, n)).astype(np.float64)
    if f["family"] == "normal":
        terms = np.stack([dz, dz * np.asarray(f["eps"], np.float64)], -1)
        return terms.sum(0), np.abs(terms).sum(0), zero
    inline = f.get("dgrad") is None
    if inline:
        from tests import implicit_grad_cases as cases
        factors = cases.reference_beta_factors(f["draws"], f["p0"], f["p1"])
    else:
        factors = np.asarray(f["dgrad"], np.float64)
    # a zero upstream never meets the factor (rows the kernel skips)
    terms = np.where((dz != 0.0)[..., None], dz[..., None] * factors, 0.0)
    absum = np.abs(terms).sum(0)
    return terms.sum(0), absum, (4.0 * floor * absum if inline else zero)


def reduce_job(job, K):
    """total [K] (float32-rounded, None for a particle-summed job), site_lp [num_sites, K],
    slot_grad [num_slots, K] (float32-rounded) as Q, and the job's particle-summed part of the loss
    (before g0) with its absolute sum."""
    sums, absums = [], []
    for v in job["values"]:
        if isinstance(v, dict):   # rank-one: f[k] * sum_seg u[seg] + e[k]
            u, f, e = (np.asarray(v[k], np.float64) for k in ("u", "f", "e"))
            sums.append(f * u.sum() + e)
            absums.append(np.abs(f) * np.abs(u).sum() + np.abs(e))
        else:
            x = np.asarray(v, np.float64)
            sums.append(x.sum(0))
            absums.append(np.abs(x).sum(0))
    ns, nl = job["num_sites"], job["num_slots"]
    scale = np.asarray(job["scale"], np.float64)
    out = {"total": None, "site_lp": None, "slot_grad": None, "ksum": 0.0, "ksum_abs": 0.0}
    if job.get("ksum") is not None:
        d = np.asarray(job["ksum"], np.float64)
        out["ksum"] = float((scale * d.sum(1)).sum())
        out["ksum_abs"] = float((np.abs(scale) * np.abs(d).sum(1)).sum())
        slots = list(zip(sums, absums))
    else:
        lp = np.stack([scale[v] * sums[v] for v in range(ns)])
        lp_abs = np.stack([abs(scale[v]) * absums[v] for v in range(ns)])
        out["site_lp"] = _q(lp, sum64=lp_abs)
        out["total"] = _q(lp.sum(0), sum64=lp_abs.sum(0))
        slots = list(zip(sums[ns:], absums[ns:]))
    if nl:
        ss = float(job["slot_scale"])
        out["slot_grad"] = _q(np.stack([s * ss for s, _ in slots]),
                              sum64=np.stack([a * abs(ss) for _, a in slots]))
    return out


def elbo_reference(case, u=None, floor=0.0, linear=()):
    """
    The forward's outputs, and with `u` (the upstream gradient, a float32 value) the backward's:
      loss, jobs [per job: total, site_lp, slot_grad], saved [per forward-absorbed Beta factor:
      [n, 4]], dterm, grads [per factor: [n, 2]], buffers [float32 arrays, exact].
    floor: tests.implicit_grad_cases.device_floor(), for factors whose implicit gradients the
    launch evaluates inline. linear: the factors whose sources enter one by one (draw_sums).
    """
    K = int(case["K"])
    g0 = float(f32(case["g0"]))
    es = float(case["entropy_scale"])
    out = {}
    lp = sum(float(np.asarray(t, np.float64).sum()) for t in case.get("terms", []))
    lp_abs = sum(float(np.abs(np.asarray(t, np.float64)).sum()) for t in case.get("terms", []))
    extra = 0.0
    out["jobs"] = []
    for job in case.get("jobs", []):
        r = reduce_job(job, K)
        out["jobs"].append(r)
        if r["total"] is not None:
            t32 = r["total"].value.astype(f32).astype(np.float64)
            lp += float(t32.sum())
            lp_abs += float(np.abs(t32).sum())
            # (the header leaves open whether the rounded totals or their fp64 sums are added)
            extra += EPS32 * abs(g0) * float(np.abs(t32).sum())
        lp += r["ksum"]
        lp_abs += r["ksum_abs"]
    h = 0.0
    h_abs = 0.0
    mags = {k: 0.0 for k in FAMILIES}
    parts = []
    for f in case.get("factors", []):
        hf, mag, d, dmag = factor_entropy(f)
        w = es * float(f["weight"])
        h += w * float(np.sum(hf))
        h_abs += w * float(np.abs(hf).sum())
        mags[f["family"]] += w * float(np.sum(mag))
        parts.append((w, d, dmag))
    out["loss"] = _q(g0 * lp - h, mag=mags, sum64=abs(g0) * lp_abs + h_abs, extra=extra)
    out["saved"] = []
    for j, (f, (w, d, dmag)) in enumerate(zip(case.get("factors", []), parts)):
        if f["family"] == "beta" and f.get("draw") == "sources":
            s, sabs, sx = draw_sums(f, K, floor, j in linear)
            zero = np.zeros_like(d)
            out["saved"].append(_q(np.concatenate([s, d], 1),
                                   mag={"beta": np.concatenate([zero, dmag], 1)},
                                   sum64=np.concatenate([sabs, zero], 1),
                                   extra=np.concatenate([sx, zero], 1)))
        else:
            out["saved"].append(None)
    if u is None:
        return out
    uf = f32(u)
    u64 = float(uf)
    out["dterm"] = _q(u64 * g0)
    out["grads"] = []
    for j, (f, (w, d, dmag)) in enumerate(zip(case.get("factors", []), parts)):
        s, sabs, sx = draw_sums(f, K, floor, j in linear)
        chain = np.ones_like(d)
        for j in range(2):
            if f["transform"][j] == 1:
                chain[:, j] = np.asarray(f["p0" if j == 0 else "p1"], np.float64)
        g = (u64 * s - u64 * w * d) * chain
        c = np.abs(chain) * abs(u64)
        out["grads"].append(_q(g, mag={f["family"]: c * w * dmag},
                               sum64=c * (sabs + w * np.abs(d)), extra=c * sx))
    out["buffers"] = [np.asarray(b, f32) if uf == f32(1.0) else (np.asarray(b, f32) * uf).astype(f32)
                      for b in case.get("buffers", [])]
    return out
