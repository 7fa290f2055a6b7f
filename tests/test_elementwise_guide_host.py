"""
The one-noise-word guide factors on the host: which factors the native sampler declines (and that
they keep the path they had), the library's exports, and the NumPy restatement the GPU test
compares against (tests/elementwise_reference.py) checked against torch float64 at that test's own
parameter values. No kernel is launched here.
"""
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import (Cauchy, Exponential, HalfCauchy, HalfNormal, Laplace, LogNormal,
                                 Normal, TransformedDistribution)
from torch.distributions.transforms import ExpTransform

from mininf_amd import _native as nat, guide
from tests import elementwise_reference as ref
from tests import predictive_reference as pr
from tests.conftest import ROOT

K_HOST = 5


def host_factors():
    one = torch.tensor([0.5, 1.5])
    return {
        "exponential": Exponential(one), "laplace": Laplace(one, one), "cauchy": Cauchy(one, one),
        "half_cauchy": HalfCauchy(one), "half_normal": HalfNormal(one),
        "log_normal": LogNormal(one, one),
    }


class MyLogNormal(LogNormal):
    pass


def test_native_sampler_declines_what_it_does_not_draw():
    for family, factor in host_factors().items():   # float32, but host-resident
        assert type(factor) in guide._ELEMENTWISE
        assert not guide.native_elementwise(factor), family
    double = torch.tensor([0.5, 1.5], dtype=torch.float64)
    assert not guide.native_elementwise(LogNormal(double, double))
    assert not guide.native_elementwise(Exponential(double))
    assert not guide.native_elementwise(MyLogNormal(torch.zeros(2), torch.ones(2)))
    by_hand = TransformedDistribution(Normal(torch.zeros(2), torch.ones(2)), ExpTransform())
    assert not guide.native_elementwise(by_hand)
    assert not guide.native_elementwise(Normal(torch.zeros(2), torch.ones(2)))
    # the class alone decides before any parameter is looked at
    assert MyLogNormal not in guide._ELEMENTWISE and TransformedDistribution not in guide._ELEMENTWISE


@pytest.mark.parametrize("family", ref.FAMILIES + ("by_hand",))
def test_declined_factors_keep_their_path(family):
    factor = TransformedDistribution(Normal(torch.zeros(2), torch.ones(2)), ExpTransform()) \
        if family == "by_hand" else host_factors()[family]

    def config(noise=None):
        return guide.DrawConfig(K=K_HOST, seed=7, step=0, stream_id=0, particle_offset=0,
                                noise=noise)

    guide._DRAWS.clear()
    injected = torch.rand(K_HOST, 2)
    assert guide.draw(factor, config(injected)) is injected   # noise passed through as the draw
    torch.manual_seed(11)
    got = guide.draw(factor, config())
    torch.manual_seed(11)
    assert torch.equal(got, factor.rsample(torch.Size([K_HOST])))   # torch's generator
    assert guide.counts()["elementwise_draws"] == 0


def test_header_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "mininf_amd.h")).read()
    declared = set(re.findall(r"^int (mi_\w+)\(", text, flags=re.M))
    new = {"mi_elementwise_rsample", "mi_elementwise_rsample_backward_workspace_bytes",
           "mi_elementwise_rsample_backward", "mi_elementwise_entropy"}
    assert new <= declared
    assert declared == set(nat.EXPORTED_SYMBOLS)
    lib = nat.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert f"#define MI_ABI_VERSION {nat.ABI_VERSION}" in text and nat.ABI_VERSION == 18
    for family, code in ref.CODE.items():
        assert getattr(nat, "PRED_" + family.upper()) == code


def test_invalid_arguments_are_rejected_before_any_launch():
    import ctypes
    lib = nat.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    size = ctypes.c_size_t()
    for family in (nat.PRED_BERNOULLI_PROBS, nat.PRED_BERNOULLI_LOGITS, -1, 8):
        assert lib.mi_elementwise_rsample(family, p, 0, p, 0, 1, 1, 0, 0, None, 0, 0, None, p,
                                          None) == -1
        assert lib.mi_elementwise_rsample_backward(family, p, 1, 1, p, 0, p, 0, 1, 1, 0, 0, None,
                                                   0, 0, None, None, 0, p, p, None) == -1
        assert lib.mi_elementwise_entropy(family, p, 0, p, 0, 1, p, p, p, None) == -1
    code = nat.PRED_LOG_NORMAL
    assert lib.mi_elementwise_rsample(code, None, 0, p, 0, 1, 1, 0, 0, None, 0, 0, None, p,
                                      None) == -1
    assert lib.mi_elementwise_rsample(code, p, 0, None, 0, 1, 1, 0, 0, None, 0, 0, None, p,
                                      None) == -1   # a two-parameter family without b
    assert lib.mi_elementwise_rsample(code, p, 0, p, 0, 1, 1, 0, 0, None, 0, 0, None, None,
                                      None) == -1
    assert lib.mi_elementwise_rsample(code, p, 0, p, 0, 0, 1, 0, 0, None, 0, 0, None, p,
                                      None) == -1
    assert lib.mi_elementwise_rsample_backward(code, None, 1, 1, p, 0, p, 0, 1, 1, 0, 0, None, 0,
                                               0, None, None, 0, p, p, None) == -1
    assert lib.mi_elementwise_rsample_backward(code, p, 1, 1, p, 0, p, 0, 1, 1, 0, 0, None, 0, 0,
                                               None, None, 0, None, None, None) == -1
    assert lib.mi_elementwise_entropy(code, p, 0, p, 0, 1, None, p, p, None) == -1
    assert lib.mi_elementwise_rsample_backward_workspace_bytes(0, 1, ctypes.byref(size)) == -1
    assert lib.mi_elementwise_rsample_backward_workspace_bytes(1, 1, None) == -1
    # one slice needs no workspace; particle slices need two float rows each
    assert lib.mi_elementwise_rsample_backward_workspace_bytes(1, 1030, ctypes.byref(size)) == 0
    assert size.value == 0
    assert lib.mi_elementwise_rsample_backward_workspace_bytes(64, 1030, ctypes.byref(size)) == 0
    assert size.value > 0 and size.value % (2 * 1030 * 4) == 0


# ---- the restatement against torch float64 -----------------------------------------------------
def t64(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def torch_transform(family, params, v):
    """The draw as torch states it, in float64: the class's icdf where the draw is an inversion
    (the Exponential inverts 1 - u: -log(u) / rate), the explicit formula otherwise."""
    d = ref.torch_distribution(family, params)
    if family == "exponential":
        return d.icdf(1.0 - v)
    if family in ("laplace", "cauchy", "half_cauchy"):
        return d.icdf(v)
    if family == "half_normal":
        return params[0] * v.abs()
    return (params[0] + params[1] * v).exp()


def compared(family, v):
    """Away from the tangents' poles (the band the GPU test leaves out as well)."""
    return pr.tangent_compared(v) if "cauchy" in family else np.ones(v.shape, bool)


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N", ref.NS)
@pytest.mark.parametrize("layout", ("dense", "scalar"))
def test_transform_and_factors_match_torch_float64(family, N, layout):
    K = K_HOST
    params = ref.parameters(family, N, layout)
    v = ref.clamp(family, ref.noise(family, K, N))
    keep = compared(family, v)
    leaves = [t64(p).expand(K, N).clone().requires_grad_() for p in params]
    z = torch_transform(family, leaves, t64(v))
    got = ref.draw(family, params, v)
    np.testing.assert_allclose(got[keep], z.detach().numpy()[keep], rtol=1e-11, atol=0)
    z.sum().backward()
    fa, fb = ref.factors(family, params, v)
    np.testing.assert_allclose(fa[keep], leaves[0].grad.numpy()[keep], rtol=1e-11, atol=0)
    assert (fb is None) == (family not in ref.TWO_PARAMETERS)
    if fb is not None:
        np.testing.assert_allclose(fb[keep], leaves[1].grad.numpy()[keep], rtol=1e-11, atol=0)


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N", ref.ENTROPY_NS)
def test_entropy_matches_torch_float64(family, N):
    params = ref.entropy_parameters(family, N)
    leaves = [t64(p).clone().requires_grad_() for p in params]
    H = ref.torch_distribution(family, leaves).entropy().sum()
    H.backward()
    got, da, db = ref.entropy(family, params)
    np.testing.assert_allclose(got, float(H.detach()), rtol=1e-12, atol=1e-12)
    want_a = leaves[0].grad if leaves[0].grad is not None else torch.zeros(N, dtype=torch.float64)
    np.testing.assert_allclose(da, want_a.numpy(), rtol=1e-12, atol=0)
    if db is not None:
        np.testing.assert_allclose(db, leaves[1].grad.numpy(), rtol=1e-12, atol=0)


def test_guide_clamp_keeps_every_draw_inside_the_support():
    """The corners of the uniform grid: u01(0) and u01(0xFFFFFFFF) (which rounds to 1.0f)."""
    corners = pr.u01(np.array([0, 0xFFFFFFFF], np.uint32)).reshape(2, 1)
    assert corners[1, 0] == np.float32(1.0)
    for family in ref.FAMILIES:
        if family in ref.NORMAL_BASED:
            continue
        z = ref.draw(family, ref.parameters(family, 1), corners)
        assert np.isfinite(z).all(), family
        if family in ref.POSITIVE:
            assert (z > 0).all(), family
    # the predictive Exponential reads 1.0f as it is: its draw there is 0
    assert pr.exponential(np.float32(2.0), corners[1], np.float64)[0] == 0.0


def test_chosen_seed_leaves_out_at_most_the_cap():
    """From the uniforms alone: in every case of the GPU test at most LEFT_OUT_CAP of the draws lie
    within 2^-10 of a tangent's pole (expected 2^-9)."""
    for N in ref.NS:
        for K in ref.KS:
            left_out = int((~pr.tangent_compared(ref.uniforms(K, N))).sum())
            assert left_out <= ref.LEFT_OUT_CAP * K * N, (K, N, left_out)
