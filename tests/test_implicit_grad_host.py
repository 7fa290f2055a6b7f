"""
The designed grids of tests/implicit_grad_cases.py reach every regime of the implicit
reparameterisation gradients and straddle every regime boundary, and the numpy oracle
(oracle.logprob.dirichlet_grad / standard_gamma_grad) agrees with torch float64 on them -- the
polynomial band of the Beta gradient included, which tests/golden/families.npz never enters.
"""
import collections

import numpy as np
import torch

from oracle import logprob as lpf
from tests import implicit_grad_cases as cases

# a straddling pair's two regimes, from the smaller x (or alpha) to the larger
BETA_SIDES = {"level_2.5": ({"small_alpha"}, {"rational", "mid_rice", "mid_poly"}),
              "level_0.75": ({"rational", "mid_rice", "mid_poly"}, {"small_beta"}),
              "band_low": ({"mid_rice"}, {"mid_poly"}),
              "band_high": ({"mid_poly"}, {"mid_rice"})}
GAMMA_SIDES = {"x_0.8": ({"series"}, {"rational", "rice", "band"}),
               "alpha_8": ({"rational"}, {"rice", "band"}),
               "band_low": ({"rice"}, {"band"}),
               "band_high": ({"band"}, {"rice"})}


def test_beta_grid_reaches_every_regime_and_straddles_every_boundary():
    x, c1, c0 = cases.beta_grid()
    assert x.dtype == c1.dtype == c0.dtype == np.float32
    assert x.shape[1] == c1.shape[0] == c0.shape[0] == len(cases.BETA_A) * len(cases.BETA_B)
    assert ((x > 0) & (x < 1)).all()
    px, pa, pb = cases.beta_points()
    tot = (pa + pb).astype(np.float32)
    counts = collections.Counter(cases.regime(px, pa, tot).tolist())
    print("beta grid:", len(px), "points,", dict(counts))
    for name in cases.BETA_REGIMES:
        assert counts[name] >= 40, (name, counts)
    # the padded grid the GPU tests launch holds the same points, so the same regimes
    full = set(zip(x.ravel().tolist(), np.broadcast_to(c1, x.shape).ravel().tolist(),
                   np.broadcast_to(c0, x.shape).ravel().tolist()))
    assert full == set(zip(px.tolist(), pa.tolist(), pb.tolist()))
    seen = collections.Counter()
    for lo, hi, a, t, kind, star, b in cases.beta_straddles():
        assert lo < star < hi
        r_lo, r_hi = str(cases.regime(lo, a, t)), str(cases.regime(hi, a, t))
        assert r_lo in BETA_SIDES[kind][0] and r_hi in BETA_SIDES[kind][1], (kind, a, t, r_lo, r_hi)
        column = cases.beta_column(a, b)
        assert np.float32(lo) in column and np.float32(hi) in column
        seen[kind, r_lo, r_hi] += 1
    # every pair of regimes that meets at a boundary is straddled somewhere
    for want in (("level_2.5", "small_alpha", "rational"), ("level_2.5", "small_alpha", "mid_rice"),
                 ("level_0.75", "rational", "small_beta"), ("level_0.75", "mid_rice", "small_beta"),
                 ("band_low", "mid_rice", "mid_poly"), ("band_high", "mid_poly", "mid_rice")):
        assert seen[want] >= 1, (want, seen)


def test_gamma_grid_reaches_every_regime_and_straddles_every_boundary():
    alpha, x = cases.gamma_grid()
    assert alpha.dtype == x.dtype == np.float32 and alpha.shape == x.shape
    assert (x > 0).all()
    counts = collections.Counter(cases.gamma_regime(alpha, x).tolist())
    print("gamma grid:", len(x), "points,", dict(counts))
    for name in cases.GAMMA_REGIMES:
        assert counts[name] >= 20, (name, counts)
    points = set(zip(alpha.astype(np.float64).tolist(), x.astype(np.float64).tolist()))
    seen = collections.Counter()
    for a_lo, x_lo, a_hi, x_hi, kind in cases.gamma_straddles():
        assert (a_lo, x_lo) in points and (a_hi, x_hi) in points
        r_lo, r_hi = str(cases.gamma_regime(a_lo, x_lo)), str(cases.gamma_regime(a_hi, x_hi))
        assert r_lo in GAMMA_SIDES[kind][0] and r_hi in GAMMA_SIDES[kind][1], (kind, a_lo, x_lo)
        seen[kind, r_lo, r_hi] += 1
    for want in (("x_0.8", "series", "rational"), ("x_0.8", "series", "rice"),
                 ("alpha_8", "rational", "rice"), ("alpha_8", "rational", "band"),
                 ("band_low", "rice", "band"), ("band_high", "band", "rice")):
        assert seen[want] >= 1, (want, seen)


def test_oracle_dirichlet_grad_matches_torch_float64_in_every_regime():
    """
    1e-11 relative; measured 1.8e-13 at worst (CPU, this grid). The margin allows for another libm
    in the pow / log1p chains.
    """
    x, c1, c0 = cases.beta_grid()
    want = cases.reference_beta_factors(x, c1, c0)
    assert np.isfinite(want).all()
    err = cases.relative_error(cases.oracle_beta_factors(x, c1, c0), want)
    tot = (c1 + c0).astype(np.float32)
    k, i, j = np.unravel_index(err.argmax(), err.shape)
    print(f"oracle dirichlet_grad vs torch float64: worst {err.max():.2e} at x={x[k, i]!r} "
          f"c1={c1[i]!r} c0={c0[i]!r} component {j} ({cases.regime(x[k, i], c1[i], tot[i])})")
    assert err.max() <= 1e-11
    labels = cases.regime(x, c1[None, :], tot[None, :])
    for name in cases.BETA_REGIMES:   # the first component's regime is the label
        assert err[..., 0][labels == name].max() <= 1e-11, name


def test_oracle_standard_gamma_grad_matches_torch_float64_in_every_regime():
    """1e-11 relative; measured 6.5e-14 at worst (CPU, this grid)."""
    alpha, x = cases.gamma_grid()
    a64, x64 = alpha.astype(np.float64), x.astype(np.float64)
    want = torch._standard_gamma_grad(torch.as_tensor(a64), torch.as_tensor(x64)).numpy()
    assert np.isfinite(want).all()
    err = cases.relative_error(lpf.standard_gamma_grad(a64, x64), want)
    i = int(err.argmax())
    print(f"oracle standard_gamma_grad vs torch float64: worst {err.max():.2e} at "
          f"alpha={alpha[i]!r} x={x[i]!r} ({cases.gamma_regime(alpha[i], x[i])})")
    assert err.max() <= 1e-11


def test_device_digamma_restatement_and_floor():
    """
    The numpy restatement of the device digamma differs from scipy's by the series' truncation
    (about 1e-11 absolute at the switch to the series), and the floor it leaves on the Beta factors
    stays 100x below the smallest regime discontinuity the grid straddles after the 4x allowance of
    the device test.
    """
    from scipy import special
    for a in (1e-6, 0.5, 1.0, 5.9, 6.0, 6.1, 40.0, 1e3):
        assert abs(cases.device_digamma(a) - special.digamma(a)) <= \
            2e-11 + 4e-16 * abs(special.digamma(a))
    floor, jump = cases.device_floor(), cases.smallest_beta_jump()
    print(f"device floor {floor:.2e}, smallest straddled jump {jump:.2e}")
    assert 0.0 < floor <= 1e-8
    assert 100.0 * 4.0 * floor <= jump
