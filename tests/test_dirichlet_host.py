"""
Dirichlet, host side (no GPU): classification of sites and guide factors, the declared entry
points, ParameterizedDistribution, and the float64 references the GPU tests compare against.
"""
import os
import re

import pytest
import torch
from torch.distributions import Dirichlet

import mininf_amd as mi
from mininf_amd import _native as nat, guide, particles
from tests import dirichlet_reference as ref
from tests.conftest import ROOT

ENTRY_POINTS = ["mi_dirichlet_forward", "mi_dirichlet_workspace_bytes", "mi_dirichlet_rsample",
                "mi_dirichlet_rsample_backward", "mi_dirichlet_rsample_backward_workspace_bytes",
                "mi_dirichlet_entropy"]


class MyDirichlet(Dirichlet):
    pass


def test_classify_dirichlet_site():
    family, roles = particles.classify(Dirichlet(torch.tensor([0.5, 2.0, 3.0])))
    assert family == "dirichlet" and len(roles) == 1
    assert roles[0].shape == (3,)
    # a subclass may override log_prob; float64 and C > MI_DIRICHLET_MAX_C keep the torch path
    assert particles.classify(MyDirichlet(torch.ones(3)))[0] == "torch"
    assert particles.classify(Dirichlet(torch.ones(3, dtype=torch.float64)))[0] == "torch"
    assert particles.classify(Dirichlet(torch.ones(nat.DIRICHLET_MAX_C)))[0] == "dirichlet"
    assert particles.classify(Dirichlet(torch.ones(nat.DIRICHLET_MAX_C + 1)))[0] == "torch"


def test_native_dirichlet_declines():
    assert nat.DIRICHLET_MAX_C == 1024
    host = Dirichlet(torch.tensor([1.0, 2.0, 3.0]))
    assert not guide.native_dirichlet(host)                                   # host-resident
    assert not guide.native_dirichlet(MyDirichlet(torch.ones(3)))             # subclass
    assert not guide.native_dirichlet(Dirichlet(torch.ones(3, dtype=torch.float64)))
    assert not guide.native_dirichlet(torch.distributions.Normal(0.0, 1.0))
    # such a guide still draws through torch (the global generator)
    for factor in (host, MyDirichlet(torch.ones(3)), Dirichlet(torch.ones(3).double())):
        cfg = guide.DrawConfig(K=5, seed=1, step=0, stream_id=0, particle_offset=0)
        torch.manual_seed(7)
        x = guide.draw(factor, cfg)
        torch.manual_seed(7)
        assert torch.equal(x, factor.rsample(torch.Size([5])))
    assert guide.counts()["dirichlet_draws"] == 0


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mininf_amd.h")).read()
    embedded = open(os.path.join(ROOT, "mininf_amd", "csrc", "embedded_header.inc")).read()
    for text in (header, embedded):
        declared = set(re.findall(r"^int (mi_\w+)\(", text, flags=re.M))
        assert set(ENTRY_POINTS) <= declared
        assert "#define MI_DIRICHLET_MAX_C 1024" in text
        assert "#define MI_ABI_VERSION 18" in text
    assert set(ENTRY_POINTS) <= set(nat.EXPORTED_SYMBOLS)
    assert nat.ABI_VERSION == 18
    lib = nat.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_entry_points_reject_bad_shapes():
    import ctypes
    lib = nat.lib()
    size = ctypes.c_size_t()
    assert lib.mi_dirichlet_workspace_bytes(0, 1, 3, ctypes.byref(size)) == nat.MI_EINVAL
    assert lib.mi_dirichlet_workspace_bytes(1, 1, 0, ctypes.byref(size)) == nat.MI_EINVAL
    assert lib.mi_dirichlet_workspace_bytes(4, 5, 3, ctypes.byref(size)) == 0
    assert size.value == 4 * 5 * 8
    assert lib.mi_dirichlet_workspace_bytes(1, 1, 1025, ctypes.byref(size)) == nat.MI_EUNSUPPORTED
    assert lib.mi_dirichlet_rsample_backward_workspace_bytes(
        7, 5, 1025, ctypes.byref(size)) == nat.MI_EUNSUPPORTED
    assert lib.mi_dirichlet_rsample_backward_workspace_bytes(7, 5, 3, ctypes.byref(size)) == 0
    assert size.value >= 7 * 5 * 8 + 5 * 8 + 5 * 4
    assert lib.mi_dirichlet_rsample(None, 1, 1, 3, 0, 0, None, 0, 0, None, None,
                                    None) == nat.MI_EINVAL
    assert lib.mi_dirichlet_entropy(None, 1, 3, None, None, None) == nat.MI_EINVAL


def test_parameterized_dirichlet_on_cpu():
    module = mi.nn.ParameterizedDistribution(Dirichlet, concentration=torch.ones(3))
    distribution = module()
    assert type(distribution) is Dirichlet
    assert distribution.concentration.device.type == "cpu"
    torch.testing.assert_close(distribution.concentration, torch.ones(3))
    assert distribution.concentration.requires_grad
    assert list(module.distribution_parameters) == ["concentration"]


def _rows(N, C, seed):
    gen = torch.Generator().manual_seed(seed)
    choices = torch.tensor([0.3, 1.0, 2.5, 40.0])
    return choices[torch.randint(0, 4, (N, C), generator=gen)]


@pytest.mark.parametrize("C", [1, 3, 65])
def test_reference_log_prob_matches_torch(C):
    conc = _rows(5, C, 0).double().requires_grad_()
    x = Dirichlet(conc.detach()).sample((7,)).clamp_min(1e-30).requires_grad_()
    want = Dirichlet(conc).log_prob(x)
    got = ref.log_prob(conc, x)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    total, da, dx = ref.density(conc.detach().expand(7, 5, C), x.detach(), scale=2.5, g0=-0.125)
    wa, wx = torch.autograd.grad(want.sum() * 2.5 * -0.125, [conc, x])
    torch.testing.assert_close(total, want.detach().sum(-1) * 2.5, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(da.sum(0), wa, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dx, wx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("C", [1, 2, 64])
def test_reference_entropy_matches_torch(C):
    conc = _rows(5, C, 1).double().requires_grad_()
    want = Dirichlet(conc).entropy().sum()
    got = ref.entropy(conc)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    (g,) = torch.autograd.grad(got, conc)
    (w,) = torch.autograd.grad(want, conc)
    torch.testing.assert_close(g, w, rtol=1e-12, atol=1e-12)


def test_reference_injected_draw_matches_torch_rsample_backward():
    torch.manual_seed(3)
    conc = _rows(5, 7, 2).double().requires_grad_()
    x = Dirichlet(conc).rsample(torch.Size([9]))          # torch's own _Dirichlet node
    weights = torch.randn(9, 5, 7, dtype=torch.float64)
    (want,) = torch.autograd.grad((x * weights).sum(), conc)
    again = conc.detach().clone().requires_grad_()
    y = ref.injected_draw(again, x.detach())
    (got,) = torch.autograd.grad((y * weights).sum(), again)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    # normalise(): rows sum to one and reproduce x from its own gamma-like multiples
    g = (x.detach() * 3.7).float()
    torch.testing.assert_close(ref.normalise(g), x.detach(), rtol=1e-6, atol=1e-12)


def test_masked_observation_is_recorded_by_rows():
    """A MaskedTensor observation of a Dirichlet site: the recorded mask has one entry per row, set
    when all the row's categories are observed."""
    y = Dirichlet(torch.ones(4)).sample((6,))
    mask = torch.ones(6, 4, dtype=torch.bool)
    mask[2] = False
    mask[4, 1] = False

    def model():
        a = mi.sample("a", torch.distributions.Gamma(2.0, 1.0), sample_shape=[4])
        mi.sample("y", Dirichlet(a), sample_shape=[6])

    conditioned = mi.condition(model, y=torch.masked.as_masked_tensor(y, mask))
    trace = particles.trace_particles(conditioned, {"a": torch.rand(3, 4) + 0.5}, 3)
    site = [s for s in trace.sites if s.name == "y"][0]
    assert site.family == "dirichlet" and tuple(site.site_shape) == (6,)
    assert site.mask.tolist() == [True, True, False, True, False, True]
    assert trace.fallback == []
