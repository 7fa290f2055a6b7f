"""
Designed evaluation points for the implicit reparameterisation gradients (csrc/beta_grad.hpp:
dirichlet_grad, standard_gamma_grad) and their float64 references.

The grids are built so that every regime of both piecewise functions is populated and every regime
boundary has a point on either side of it. Points sit beside a boundary, never on it: the kernels
may contract total * x * (1 - x) differently from the host by an ulp, and a point exactly on a
boundary would test nothing. Every value is rounded to float32 first, and the Beta total is the
float32 sum of the float32 concentrations, as in the kernels (dirichlet.py:18).
"""
from __future__ import annotations

import functools
import math
import types
from unittest import mock

import numpy as np
import torch

from oracle import logprob as lpf

f32 = np.float32

BETA_A = (0.05, 0.3, 1.0, 2.5, 5.9, 6.1, 8.0, 40.0, 300.0, 3000.0)
BETA_B = (0.05, 0.4, 1.0, 3.0, 5.9, 6.1, 12.0, 50.0, 700.0)
BETA_REGIMES = ("small_alpha", "small_beta", "mid_rice", "mid_poly", "rational")
BAND_EDGE_MAX = 40.0   # band-edge points only up to here: beyond, the jump across the edge shrinks
                       # (1e-6 at 300, 1e-8 at 3000) towards the device's own rounding floor
X_TOP = f32(1.0) - f32(2.0 ** -24)   # the largest float32 below 1

GAMMA_ALPHA = (0.01, 0.3, 1.0, 2.5, float(np.nextafter(f32(8), f32(0))), 8.0,
               float(np.nextafter(f32(8), f32(9))), 8.5, 40.0, 1000.0, 1e4)
GAMMA_REGIMES = ("series", "rational", "rice", "band")


def _neighbours(v):
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


def regime(x, a, tot):
    """
    The regime of dirichlet_grad(x, a, tot), classified in float64 from the (float32-rounded)
    values. Vectorised; returns an array of names from BETA_REGIMES.
    """
    x, a, tot = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (x, a, tot)))
    b = tot - a
    boundary = tot * x * (1.0 - x)
    mean = a / tot
    sd = np.sqrt(a * b / (tot + 1.0)) / tot
    band = (mean - 0.1 * sd <= x) & (x <= mean + 0.1 * sd)
    out = np.where((a > 6.0) & (b > 6.0), np.where(band, "mid_poly", "mid_rice"), "rational")
    out = np.where((x >= 0.5) & (boundary < 0.75), "small_beta", out)
    return np.where((x <= 0.5) & (boundary < 2.5), "small_alpha", out)


def regime_value(name, x, a, tot):
    """The formula of regime `name` evaluated at one point, whether or not the point is in it."""
    x, a, tot = float(x), float(a), float(tot)
    b = tot - a
    if name == "small_alpha":
        return lpf._grad_small_alpha(x, a, b)
    if name == "small_beta":
        return -lpf._grad_small_beta(1 - x, b, a)
    if name == "mid_poly":
        return lpf._grad_mid_poly(x, a, b)
    if name == "mid_rice":
        return lpf._grad_mid_rice(x, a, b)
    return lpf._grad_rational(x, a, tot)


@functools.lru_cache(maxsize=None)
def _beta_columns():
    """Per (a, b) pair: (a32, b32, tot32, unique float32 x values, straddling pairs)."""
    columns = []
    for a in BETA_A:
        for b in BETA_B:
            a32, b32 = f32(a), f32(b)
            tot32 = f32(a32 + b32)
            av, tv = float(a32), float(tot32)
            bv = tv - av
            xs = [f32(v) for v in (1e-30, 1e-6, 1e-4, 0.02, 0.3)] + _neighbours(0.5) + \
                [f32(v) for v in (0.7, 0.98, 0.9999)] + [X_TOP]
            pairs = []   # (x below, x above, the boundary between them, boundary kind)
            mean = av / tv
            sd = math.sqrt(av * bv / (tv + 1.0)) / tv
            edges = max(a, b) <= BAND_EDGE_MAX
            band = {s: f32(mean + s * sd) for s in ((-0.11, -0.09, 0.0, 0.09, 0.11) if edges
                                                    else (0.0,))}
            xs += list(band.values())
            # inside the band, away from its edges, for every pair
            xs += [f32(mean - 0.05 * sd), f32(mean + 0.05 * sd)]
            if edges and av > 6.0 and bv > 6.0:
                pairs += [(band[-0.11], band[-0.09], mean - 0.1 * sd, "band_low"),
                          (band[0.09], band[0.11], mean + 0.1 * sd, "band_high")]
            for level in (2.5, 0.75):
                disc = 1.0 - 4.0 * level / tv
                if disc <= 0.0:
                    continue
                for root in (0.5 * (1.0 - math.sqrt(disc)), 0.5 * (1.0 + math.sqrt(disc))):
                    lo, hi = f32(root * (1.0 - 1e-5)), f32(root * (1.0 + 1e-5))
                    xs += [lo, hi]
                    # the 2.5 level bounds small_alpha (x <= 0.5), the 0.75 level small_beta
                    # (x >= 0.5); the other two roots are plain extra points
                    if (level == 2.5) == (root < 0.5):
                        pairs.append((lo, hi, root, f"level_{level}"))
            xs = [v for v in xs if 0.0 < v < 1.0]
            unique = list(dict.fromkeys(float(v) for v in xs))
            columns.append((a32, b32, tot32, np.asarray(unique, f32), pairs))
    return columns


def beta_grid():
    """x [K, N], c1 [N], c0 [N] (float32): column i holds the points of pair i, padded to the
    common K by repeating its last x."""
    cols = _beta_columns()
    K = max(len(c[3]) for c in cols)
    x = np.stack([np.concatenate([c[3], np.full(K - len(c[3]), c[3][-1], f32)]) for c in cols], 1)
    return (np.ascontiguousarray(x, f32), np.asarray([c[0] for c in cols], f32),
            np.asarray([c[1] for c in cols], f32))


def beta_points():
    """The grid without its padding, flattened along N: x [M], c1 [M], c0 [M] (float32)."""
    cols = _beta_columns()
    return (np.concatenate([c[3] for c in cols]),
            np.concatenate([np.full(len(c[3]), c[0], f32) for c in cols]),
            np.concatenate([np.full(len(c[3]), c[1], f32) for c in cols]))


def beta_straddles():
    """The boundary pairs the grid claims: (x_low, x_high, a, tot, kind, boundary, b) in
    float64."""
    return [(float(lo), float(hi), float(c[0]), float(c[2]), kind, star, float(c[1]))
            for c in _beta_columns() for lo, hi, star, kind in c[4]]


def beta_column(c1, c0):
    """The grid's x values (float32) for the pair (c1, c0)."""
    for a32, b32, _, xs, _ in _beta_columns():
        if a32 == f32(c1) and b32 == f32(c0):
            return xs
    raise KeyError((c1, c0))


def smallest_beta_jump():
    """
    The smallest relative discontinuity of dirichlet_grad among the grid's boundary pairs: the
    formulas of the two regimes a pair straddles, both evaluated on the boundary between them. (At
    a pair's own points the two formulas may differ by less: for (40, 6.1) they cross just inside
    the band's upper edge.)
    """
    worst = np.inf
    for lo, hi, a, tot, _, star, _ in beta_straddles():
        v_lo = regime_value(str(regime(lo, a, tot)), star, a, tot)
        v_hi = regime_value(str(regime(hi, a, tot)), star, a, tot)
        worst = min(worst, abs(v_lo - v_hi) / min(abs(v_lo), abs(v_hi)))
    return worst


def gamma_regime(alpha, x):
    """The regime of standard_gamma_grad(alpha, x), classified in float64. Vectorised."""
    alpha, x = np.broadcast_arrays(np.asarray(alpha, np.float64), np.asarray(x, np.float64))
    band = (float(f32(0.9)) * alpha <= x) & (x <= float(f32(1.1)) * alpha)
    out = np.where(alpha > 8.0, np.where(band, "band", "rice"), "rational")
    return np.where(x < float(f32(0.8)), "series", out)


@functools.lru_cache(maxsize=None)
def _gamma_points():
    alphas, xs, pairs = [], [], []
    for a in GAMMA_ALPHA:
        a32 = f32(a)
        av = float(a32)
        col = [f32(v) for v in (1e-30, 1e-6, 0.05, 0.5)] + _neighbours(0.8)
        near = []
        for centre in (float(f32(0.9)) * av, float(f32(1.1)) * av, av):
            lo, hi = f32(centre * (1.0 - 1e-5)), f32(centre * (1.0 + 1e-5))
            near.append((lo, hi))
            col += [lo, hi]
        col += [f32(0.3 * av), f32(3.0 * av), f32(av - 3.0 * math.sqrt(av)),
                f32(av + 3.0 * math.sqrt(av))]
        col = list(dict.fromkeys(float(v) for v in col if v > 0.0))
        alphas += [a32] * len(col)
        xs += col
        lo8, at8, _ = _neighbours(0.8)
        pairs.append((av, float(lo8), av, float(at8), "x_0.8"))
        if av > 8.0:
            pairs.append((av, float(near[0][0]), av, float(near[0][1]), "band_low"))
            pairs.append((av, float(near[1][0]), av, float(near[1][1]), "band_high"))
    # alpha = 8 is a boundary in alpha: the same x on either side of it
    at, above = float(f32(8)), float(np.nextafter(f32(8), f32(9)))
    for xv in (float(f32(0.3 * at)), float(f32(at * (1.0 - 1e-5))), float(f32(3.0 * at))):
        alphas += [f32(at), f32(above)]
        xs += [xv, xv]
        pairs.append((at, xv, above, xv, "alpha_8"))
    return np.asarray(alphas, f32), np.asarray(xs, f32), pairs


def gamma_grid():
    """alpha [M], x [M] (float32)."""
    alpha, x, _ = _gamma_points()
    return alpha.copy(), x.copy()


def gamma_straddles():
    """The boundary pairs the gamma grid claims: (alpha, x, alpha', x', kind) in float64."""
    return list(_gamma_points()[2])


def reference_beta_factors(x, c1, c0):
    """
    mi_beta_dgrad's factors from torch._dirichlet_grad in float64 on the CPU:
      out[..., 0] = dgrad(x, c1, c1 + c0) (1 - x),  out[..., 1] = -dgrad(1 - x, c0, c1 + c0) x
    with 1 - x and c1 + c0 formed in float32 as the kernels form them, and every input a float32
    value widened to double. x [..., N] broadcasts against c1 [N], c0 [N].
    """
    x = np.asarray(x, f32)
    c1, c0 = np.broadcast_arrays(np.asarray(c1, f32), np.asarray(c0, f32))
    c1, c0 = np.broadcast_to(c1, x.shape), np.broadcast_to(c0, x.shape)
    w = f32(1.0) - x
    tot = (c1 + c0).astype(f32)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64))   # noqa: E731
    d1 = torch._dirichlet_grad(t(x), t(c1), t(tot)).numpy() * w.astype(np.float64)
    d0 = -torch._dirichlet_grad(t(w), t(c0), t(tot)).numpy() * x.astype(np.float64)
    return np.stack([d1, d0], -1)


def oracle_beta_factors(x, c1, c0, digamma=None):
    """
    The same factors from oracle.logprob.dirichlet_grad, optionally with another digamma in place
    of scipy's (device_digamma: the measured floor of the device's fp64 factors).
    """
    x = np.asarray(x, f32)
    c1, c0 = np.broadcast_to(np.asarray(c1, f32), x.shape), np.broadcast_to(np.asarray(c0, f32),
                                                                           x.shape)
    w = (f32(1.0) - x).astype(np.float64)
    tot = (c1 + c0).astype(f32).astype(np.float64)
    x64, a, b = x.astype(np.float64), c1.astype(np.float64), c0.astype(np.float64)
    shim = lpf.special if digamma is None else types.SimpleNamespace(digamma=digamma)
    with mock.patch.object(lpf, "special", shim):
        d1 = lpf.dirichlet_grad(x64, a, tot) * w
        d0 = -lpf.dirichlet_grad(w, b, tot) * x64
    return np.stack([d1, d0], -1)


def device_digamma(x):
    """
    csrc/device_math.hpp's digamma restated for positive arguments: the recurrence up to 6, then
    the five-term asymptotic series, in float64.
    """
    x = float(x)
    shift = 0.0
    while x < 6.0:
        shift -= 1.0 / x
        x += 1.0
    r = 1.0 / (x * x)
    series = r * (1.0 / 12 - r * (1.0 / 120 - r * (1.0 / 252 - r * (1.0 / 240 - r * (1.0 / 132)))))
    return shift + math.log(x) - 0.5 / x - series


def relative_error(got, want):
    """|got - want| / |want| elementwise; 0 where both are 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.where(want == 0.0, 1.0, np.abs(want))
    return np.abs(got - want) / scale


def device_floor():
    """
    The measured floor of mi_beta_dgrad on the grid: the largest relative difference between the
    numpy oracle evaluated with the device's digamma and torch float64. The series the device
    truncates leaves about 1e-11 at the switch, amplified where psi(total) - psi(alpha) cancels.
    """
    x, c1, c0 = beta_grid()
    return float(relative_error(oracle_beta_factors(x, c1, c0, device_digamma),
                                reference_beta_factors(x, c1, c0)).max())
