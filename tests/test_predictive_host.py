"""
Predictive draws, host side (no GPU): which distributions the HIP samplers take, how the vmap rule
hands parameters to a launch, the declared entry points, and the self-consistency of the NumPy
reference (tests/predictive_reference.py) at the GPU tests' inputs: its float32 and float64
restatements differ by at most a quarter of what tests/test_gpu_predictive_families.py allows the
kernels, so each of that test's caps is a condition the reference itself meets with room.
"""
import ctypes
import types

import numpy as np
import pytest
import torch
from torch.distributions import (Bernoulli, Beta, Binomial, Categorical, Cauchy, Dirichlet,
                                 Exponential, Gamma, HalfCauchy, HalfNormal, Laplace, LogNormal,
                                 MultivariateNormal, NegativeBinomial, Normal, Poisson, StudentT)

from mininf_amd import _native as nat, predictive
from mininf_amd.distributions import InverseGamma
from tests import predictive_reference as ref

NEW = [Bernoulli(probs=torch.tensor([0.2, 0.7])), Bernoulli(logits=torch.tensor([0.2, -0.7])),
       Exponential(torch.tensor(2.0)), Laplace(torch.zeros(3), torch.ones(3)),
       Cauchy(torch.zeros(3), torch.ones(3)), HalfCauchy(torch.ones(2)), HalfNormal(torch.ones(2)),
       LogNormal(torch.zeros(2), torch.ones(2)), Poisson(torch.tensor([3.0, 40.0])),
       Categorical(logits=torch.zeros(4, 3)), Categorical(probs=torch.ones(3) / 3)]


class MyPoisson(Poisson):
    pass


class MyBernoulli(Bernoulli):
    pass


@pytest.fixture
def everywhere(monkeypatch):
    """Host tensors count as device-resident: the predicate's type and dtype part."""
    monkeypatch.setattr(predictive, "_resident", lambda t: True)


def test_supported_families(everywhere):
    for distribution in NEW + [Normal(0.0, 1.0), Gamma(2.0, 2.0), Beta(2.0, 2.0)]:
        assert predictive.supported(distribution), distribution
    declined = [MyPoisson(torch.tensor(3.0)), MyBernoulli(torch.tensor(0.3)),
                Poisson(torch.tensor(3.0, dtype=torch.float64)),
                Bernoulli(torch.tensor(0.3, dtype=torch.float64)),
                Categorical(logits=torch.zeros(3, dtype=torch.float64)),
                Categorical(logits=torch.zeros(nat.PRED_CATEGORICAL_MAX_C + 1)),
                Binomial(10, torch.tensor(0.3)), NegativeBinomial(5, torch.tensor(0.3)),
                StudentT(torch.tensor(3.0)), InverseGamma(torch.tensor(3.0), torch.tensor(1.0)),
                Dirichlet(torch.ones(3)), MultivariateNormal(torch.zeros(2), torch.eye(2))]
    for distribution in declined:
        assert not predictive.supported(distribution), distribution
    assert predictive.supported(Categorical(logits=torch.zeros(nat.PRED_CATEGORICAL_MAX_C)))


def test_host_resident_parameters_keep_torch():
    for distribution in NEW:
        assert not predictive.supported(distribution), distribution


def test_masked_parameters_keep_torch(everywhere):
    rate = torch.masked.as_masked_tensor(torch.ones(3), torch.tensor([True, False, True]))
    held = Poisson(torch.ones(3), validate_args=False)
    held.rate = rate
    assert not predictive.supported(held)


def test_bernoulli_reads_the_parameter_it_holds():
    """The other parameterisation is a lazy property; reading it would launch the conversion."""
    by_probs, by_logits = Bernoulli(probs=torch.tensor([0.2])), Bernoulli(logits=torch.tensor([0.2]))
    family, (p,) = predictive._params(by_probs)
    assert family == predictive.SAMPLE + nat.PRED_BERNOULLI_PROBS and p is by_probs.__dict__["probs"]
    assert "logits" not in by_probs.__dict__
    family, (l,) = predictive._params(by_logits)
    assert family == predictive.SAMPLE + nat.PRED_BERNOULLI_LOGITS
    assert l is by_logits.__dict__["logits"] and "probs" not in by_logits.__dict__
    assert "probs" not in Categorical(logits=torch.zeros(3)).__dict__
    family, (held,) = predictive._params(Categorical(probs=torch.ones(3) / 3))
    assert family == predictive.CATEGORICAL and "logits" not in Categorical(probs=held).__dict__


def _stubbed(monkeypatch):
    calls = []

    def launch(family, params, S, M, seed, stream_id):
        calls.append((family, params, S, M))
        return torch.zeros(S * M)

    monkeypatch.setattr(predictive, "_launch", launch)
    return calls


def test_vmap_rule_passes_strides_without_a_copy(monkeypatch):
    calls = _stubbed(monkeypatch)
    S, n = 5, 7
    info = types.SimpleNamespace(batch_size=S, randomness="different")
    index = torch.arange(S)
    family = predictive.SAMPLE + nat.PRED_BERNOULLI_PROBS
    theta = torch.rand(S)               # a per-sample scalar, drawn n times
    out, dim = predictive._DrawFn.vmap(info, (0, 0, 0, None, None, None, None), index, theta, theta,
                                       family, (n,), 1, 2)
    assert out.shape == (S, n) and dim == 0
    (_, params, gotS, gotM), = calls
    assert (gotS, gotM) == (S, n)
    tensor, ss, sj = params[0]
    assert (ss, sj) == (1, 0) and tensor.data_ptr() == theta.data_ptr()
    calls.clear()
    p = torch.rand(n)                   # a per-element constant
    predictive._DrawFn.vmap(info, (0, None, None, None, None, None, None), index, p, p, family, (),
                            1, 2)
    tensor, ss, sj = calls[0][1][0]
    assert (ss, sj) == (0, 1) and tensor.data_ptr() == p.data_ptr()
    calls.clear()
    dense = torch.rand(n, S)            # batched along its last axis: read transposed in place
    predictive._DrawFn.vmap(info, (0, 1, 1, None, None, None, None), index, dense, dense, family,
                            (), 1, 2)
    tensor, ss, sj = calls[0][1][0]
    assert (ss, sj) == (1, S) and tensor.data_ptr() == dense.data_ptr()
    calls.clear()
    # replications of a per-element constant: no stride pair over [S, 3 n] describes it, but the
    # samples share it, so one sample's 3 n values are laid out and read with stride_s = 0
    predictive._DrawFn.vmap(info, (0, None, None, None, None, None, None), index, p, p, family,
                            (3,), 1, 2)
    tensor, ss, sj = calls[0][1][0]
    assert (ss, sj) == (0, 1) and tensor.numel() == 3 * n and calls[0][3] == 3 * n


def test_single_stride_of_the_existing_entry_points():
    S, M = 4, 6
    dense = torch.rand(S, M)
    v, ss, sj = predictive._strided(dense, S, M)
    t, stride = predictive._single_stride(v, ss, sj, S, M)
    assert stride == 1 and t.data_ptr() == dense.data_ptr()
    constant = torch.tensor(2.0).expand(S, M)
    v, ss, sj = predictive._strided(constant, S, M)
    t, stride = predictive._single_stride(v, ss, sj, S, M)
    assert stride == 0 and t.data_ptr() == constant.data_ptr()
    scalar = torch.rand(S, 1).expand(S, M)   # (1, 0): materialised, as before
    v, ss, sj = predictive._strided(scalar, S, M)
    t, stride = predictive._single_stride(v, ss, sj, S, M)
    assert stride == 1 and torch.equal(t, scalar)


def test_categorical_rule_keeps_the_category_axis(monkeypatch):
    calls = []

    def launch(logits, strides, S, T, B, C, seed, stream_id):
        calls.append((logits, strides, S, T, B, C))
        return torch.zeros(S * T * B, dtype=torch.int64)

    monkeypatch.setattr(predictive, "_launch_categorical", launch)
    S = 5
    info = types.SimpleNamespace(batch_size=S, randomness="different")
    logits = torch.randn(S, 3)
    out, _ = predictive._CategoricalFn.vmap(info, (0, 0, None, None, None), torch.arange(S), logits,
                                            (4,), 1, 2)
    assert out.shape == (S, 4) and out.dtype == torch.int64
    tensor, strides, *sizes = calls[0]
    assert sizes == [S, 4, 1, 3] and strides == (3, 0, 1) and tensor.data_ptr() == logits.data_ptr()
    shared = torch.randn(2, 3)
    out, _ = predictive._CategoricalFn.vmap(info, (0, None, None, None, None), torch.arange(S),
                                            shared, (), 1, 2)
    tensor, strides, *sizes = calls[1]
    assert out.shape == (S, 2) and sizes == [S, 1, 2, 3] and strides == (0, 3, 1)
    assert tensor.data_ptr() == shared.data_ptr()


def test_counters():
    predictive.reset_counts()
    assert predictive.native_draws() == {}
    snapshot = predictive.native_draws()
    snapshot["Poisson"] += 2
    assert predictive.native_draws()["Poisson"] == 0   # a copy
    predictive.reset_counts(snapshot)
    assert predictive.native_draws()["Poisson"] == 2
    predictive.reset_counts()


def test_entry_points_reject_bad_sizes():
    lib = nat.lib()
    buf = (ctypes.c_float * 4)()
    out = (ctypes.c_int64 * 4)()
    p, o = ctypes.addressof(buf), ctypes.addressof(out)
    assert lib.mi_predictive_sample(0, None, 0, 0, None, 0, 0, 1, 1, 0, 0, p, None) == nat.MI_EINVAL
    assert lib.mi_predictive_sample(8, p, 0, 0, None, 0, 0, 1, 1, 0, 0, p, None) == nat.MI_EINVAL
    assert lib.mi_predictive_sample(nat.PRED_LAPLACE, p, 0, 0, None, 0, 0, 1, 1, 0, 0, p,
                                    None) == nat.MI_EINVAL   # scale missing
    assert lib.mi_predictive_sample(0, p, 0, 0, None, 0, 0, 0, 1, 0, 0, p, None) == nat.MI_EINVAL
    assert lib.mi_predictive_sample(0, p, 0, 0, None, 0, 0, 1 << 20, (1 << 14) + 1, 0, 0, p,
                                    None) == nat.MI_EUNSUPPORTED   # N > 2^34
    assert lib.mi_predictive_sample(0, p, 0, 0, None, 0, 0, 1 << 62, 1 << 62, 0, 0, p,
                                    None) == nat.MI_EUNSUPPORTED   # (no overflow on the way)
    assert lib.mi_predictive_categorical(p, 0, 0, 1, 1, 1, 1, 0, 0, 0, o, None) == nat.MI_EINVAL
    assert lib.mi_predictive_categorical(p, 0, 0, 1, 1, 1, 1, 1025, 0, 0, o,
                                         None) == nat.MI_EUNSUPPORTED
    assert lib.mi_predictive_categorical(p, 0, 0, 1, 1 << 20, 1 << 10, 1 << 5, 3, 0, 0, o,
                                         None) == nat.MI_EUNSUPPORTED   # rows > 2^34
    assert lib.mi_predictive_categorical(None, 0, 0, 1, 1, 1, 1, 3, 0, 0, o, None) == nat.MI_EINVAL
    assert lib.mi_predictive_poisson(p, 0, 0, 1, 0, 0, 0, p, None) == nat.MI_EINVAL
    assert lib.mi_predictive_poisson(p, 0, 0, 1 << 20, (1 << 12) + 1, 0, 0, p,
                                     None) == nat.MI_EUNSUPPORTED   # N > 2^32
    assert lib.mi_predictive_poisson(p, 0, 0, 1, 1, 0, 1 << 24, p, None) == nat.MI_EINVAL


# ---- the reference against itself -----------------------------------------------------------------
# The GPU test's caps: relative error 1e-4 (its bounds are no looser), 1 % of draws marked.
RTOL_CAP, MARKED_CAP = 1e-4, 0.01


def test_uniforms_are_the_oracles():
    """The restated words are the generator's: Box-Muller on them gives oracle_guide_normals."""
    from oracle import build as oracle_build
    n = 1001
    want = np.empty(n, np.float32)
    oracle_build.load().oracle_guide_normals(1, n, ref.SEED, 0, 7, 0, want.ctypes.data)
    np.testing.assert_allclose(ref.normals(ref.SEED, 7, n), want, rtol=0, atol=1e-6)
    u = ref.uniforms(ref.SEED, 7, n)
    assert u.dtype == np.float32 and 0 < u.min() and u.max() <= 1


@pytest.mark.parametrize("family", sorted(ref.FIXED))
def test_fixed_families_float32_against_float64(family):
    worst, flips, marks, draws, left_out = 0.0, 0, 0, 0, 0
    for S, M in ref.SHAPES:
        for layout in ref.LAYOUTS:
            params = ref.fixed_parameters(family, S, M, layout)
            want, marked, u = ref.fixed_draw(family, params, ref.SEED, ref.FIXED_STREAM, S, M, np.float64)
            got, _, _ = ref.fixed_draw(family, params, ref.SEED, ref.FIXED_STREAM, S, M, np.float32)
            draws += S * M
            if family.startswith("bernoulli"):
                keep = ~marked if marked is not None else np.ones((S, M), bool)
                assert np.array_equal(got[keep], want[keep])
                flips += int((got != want).sum())
                marks += int(marked.sum()) if marked is not None else 0
                continue
            keep = ref.tangent_compared(u) if "cauchy" in family else np.ones((S, M), bool)
            left_out += int((~keep).sum())
            params_b = [np.broadcast_to(p, (S, M))[keep] for p in params]
            worst = max(worst, float(ref.relative_error(family, params_b, got[keep],
                                                        want[keep]).max()))
    assert worst <= RTOL_CAP / 4, worst
    assert left_out <= 0.002 * draws, (left_out, draws)
    assert flips <= MARKED_CAP / 4 * draws and marks <= MARKED_CAP * draws


def test_categorical_float32_against_float64():
    flips = marks = draws = 0
    for C, B, T in ref.CATEGORICAL_CASES:
        rows = ref.categorical_rows(ref.categorical_logits(C, B), T)
        u = ref.uniforms(ref.SEED, 11, len(rows))
        want, marked = ref.categorical(rows, u, np.float64)
        got, _ = ref.categorical(rows, u, np.float32)
        assert np.array_equal(got[~marked], want[~marked]), (C, B, T)
        assert want.min() >= 0 and want.max() < C and np.isfinite(rows[np.arange(len(rows)), want]).all()
        flips, marks, draws = flips + int((got != want).sum()), marks + int(marked.sum()), \
            draws + len(rows)
    assert marks <= MARKED_CAP * draws and flips <= MARKED_CAP / 4 * draws, (marks, flips, draws)


def test_poisson_float32_against_float64():
    rates = ref.poisson_rates().reshape(-1)
    want, marked, blocks = ref.poisson(rates, ref.SEED, 9, np.float64)
    got, _, _ = ref.poisson(rates, ref.SEED, 9, np.float32)
    assert np.array_equal(got[~marked], want[~marked])
    assert marked.mean() <= MARKED_CAP and (got != want).mean() <= MARKED_CAP / 4
    assert blocks.max() <= 64 and (want[rates == 0] == 0).all()
    # the draws are Poisson: mean and variance of each rate within 5 standard errors
    for rate in ref.POISSON_RATES[1:]:
        x, n = want[rates == rate], int((rates == rate).sum())
        assert abs(x.mean() - rate) < 5 * np.sqrt(rate / n), rate
        assert abs(x.var(ddof=1) - rate) < 5 * np.sqrt((rate + 2.0 * rate * rate) / n), rate
    bad, _, _ = ref.poisson(np.array([-1.0, np.nan, np.inf], np.float32), ref.SEED, 9)
    assert np.isnan(bad).all()
