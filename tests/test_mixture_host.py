"""
The Normal-mixture site on the host (no GPU): the float64 closed form the GPU tests compare
against equals torch's own MixtureSameFamily.log_prob and its autograd, the tracer classifies the
qualifying type and no other, and the float32 restatement of the predictive draw chooses the
float64 one's component wherever the uniform is not within rounding of a cumulative boundary.
"""
import numpy as np
import pytest
import torch
from torch.distributions import (Categorical, Gamma, Independent, MixtureSameFamily, Normal)

import mininf_amd as mi
from mininf_amd import _native as nat, particles, predictive
from tests import mixture_reference as mref


def mixture(C, dtype=torch.float32, batch=()):
    return MixtureSameFamily(Categorical(probs=torch.ones(batch + (C,), dtype=dtype) / C),
                             Normal(torch.zeros(batch + (C,), dtype=dtype),
                                    torch.ones(batch + (C,), dtype=dtype)))


class MyMixture(MixtureSameFamily):
    pass


CASES = [(C, N, K, layout) for C in mref.KERNEL_C for N, K in ((1, 1), (5, 7))
         for layout in mref.LAYOUTS if not (C == 1024 and layout != "dense")]


@pytest.mark.parametrize("C, N, K, layout", CASES)
def test_closed_form_is_torchs_float64(C, N, K, layout):
    inputs = mref.kernel_case(C, N, K, layout)
    mask = np.arange(N) % 3 != 1 if N > 1 else None
    want = mref.closed_form(*inputs, mask=mask, batch_scale=2.5, g0=-1.0 / K)
    got = mref.torch_float32(*inputs, mask=mask, batch_scale=2.5, g0=-1.0 / K,
                             dtype=torch.float64)
    for name in ("total",) + mref.GRADS:
        np.testing.assert_allclose(got[name], want[name], rtol=1e-12, atol=1e-12, err_msg=name)


def test_closed_form_special_rows():
    # a -inf logit: exact zeros, nothing NaN; a row 40 standard deviations away: finite, sum r = 1
    logits, loc, scale, x = mref.kernel_case(5, 3, 2)
    logits = logits.copy()
    logits[:, :, 2] = -np.inf
    want = mref.closed_form(logits, loc, scale, x)
    for name in mref.GRADS[:3]:
        assert np.all(want[name][:, :, 2] == 0)
    assert all(np.isfinite(want[name]).all() for name in ("total",) + mref.GRADS)
    far = mref.closed_form(*mref.far_case())
    assert np.isfinite(far["row"]).all() and far["row"][:, 1].max() < -700
    np.testing.assert_allclose(far["r"].sum(-1), 1.0, rtol=1e-12)


def test_classification():
    family, roles = particles.classify(mixture(3))
    assert family == "mixture_normal" and len(roles) == 3
    d = mixture(3)
    family, roles = particles.classify(d)
    assert roles[0] is d.mixture_distribution.logits
    assert roles[1] is d.component_distribution.loc and roles[2] is d.component_distribution.scale
    assert particles.classify(mixture(nat.MIXTURE_MAX_C))[0] == "mixture_normal"
    assert nat.MIXTURE_MAX_C == 1024
    declined = [
        MyMixture(Categorical(probs=torch.ones(3) / 3), Normal(torch.zeros(3), torch.ones(3))),
        MixtureSameFamily(Categorical(probs=torch.ones(3) / 3),
                          Independent(Normal(torch.zeros(3, 2), torch.ones(3, 2)), 1)),
        MixtureSameFamily(Categorical(probs=torch.ones(3) / 3),
                          Gamma(torch.ones(3), torch.ones(3))),
        mixture(3, torch.float64),
        mixture(nat.MIXTURE_MAX_C + 1),
    ]
    for d in declined:
        assert particles.classify(d) == ("torch", []), d


@pytest.mark.parametrize("shared", [False, True])
def test_site_shape(shared):
    K, n, C = 4, 6, 3
    x = torch.randn(n)

    def model():
        mu = mi.sample("mu", Normal(0.0, 5.0), sample_shape=[C] if shared else [n, C])
        w = torch.ones(C) / C
        mi.sample("x", MixtureSameFamily(Categorical(probs=w), Normal(mu, torch.ones(C))),
                  sample_shape=[n] if shared else None)

    samples = {"mu": torch.randn((K, C) if shared else (K, n, C))}
    trace = particles.trace_particles(mi.condition(model, x=x), samples, K)
    assert trace.fallback == []
    site = trace.sites[-1]
    assert site.family == "mixture_normal" and tuple(site.site_shape) == (n,)
    assert len(site.roles) == 4 and site.description == "MixtureSameFamily"
    assert tuple(site.tensors[1].shape) == ((K, C) if shared else (K, n, C))
    # a float64 value keeps torch's path, as the Dirichlet branch does
    trace = particles.trace_particles(mi.condition(model, x=x.double()), samples, K)
    assert [name for name, _ in trace.fallback] == ["x"]


def test_predictive_supported(monkeypatch):
    assert not predictive.supported(mixture(3))   # host-resident parameters keep torch
    monkeypatch.setattr(predictive, "_resident", lambda t: True)
    assert predictive.supported(mixture(3)) and predictive.supported(mixture(3, batch=(4,)))
    assert predictive.supported(mixture(nat.PRED_CATEGORICAL_MAX_C))
    family, params = predictive._params(mixture(3))
    assert family == predictive.MIXTURE_NORMAL and len(params) == 3
    declined = [
        MyMixture(Categorical(probs=torch.ones(3) / 3), Normal(torch.zeros(3), torch.ones(3))),
        MixtureSameFamily(Categorical(probs=torch.ones(3) / 3),
                          Independent(Normal(torch.zeros(3, 2), torch.ones(3, 2)), 1)),
        MixtureSameFamily(Categorical(probs=torch.ones(3) / 3),
                          Gamma(torch.ones(3), torch.ones(3))),
        mixture(3, torch.float64),
        mixture(nat.PRED_CATEGORICAL_MAX_C + 1),
    ]
    for d in declined:
        assert not predictive.supported(d), d


@pytest.mark.parametrize("C", mref.DRAW_C)
def test_float32_draw_chooses_the_same_component(C):
    """A case is one component count: every shape, parameters dense and shared (what one case of
    the GPU test draws)."""
    count = total = 0
    for shared in (False, True):
        for S, T, B, _ in (case for case in mref.DRAW_CASES if case[3] == C):
            params = mref.draw_parameters(S, B, C, shared)
            args = (S, T, mref.DRAW_SEED, mref.DRAW_STREAM)
            _, want, marked, _ = mref.draw(*params, *args, np.float64)
            _, got, _, _ = mref.draw(*params, *args, np.float32)
            assert np.array_equal(got[~marked], want[~marked]), (S, T, B, C)
            count, total = count + int(marked.sum()), total + marked.size
    print(f"C={C}: {count} of {total} draws marked")
    assert count <= 0.0025 * total   # a quarter of the 1 % the GPU test allows
