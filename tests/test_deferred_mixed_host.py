"""
Calls in which a deferred ``X @ theta`` and a deferred ``alpha[group]`` meet (mininf_amd.linear), on
the host: every model is traced once with both deferrals on and once with both off, and the two
traces must record the same sites -- the family, what stays linear or gathered and with which link
-- and bit-identical tensors. Both traces issue the same torch calls on the same device, so the
comparison is ``torch.equal``; a role that stays deferred on purpose is compared after the engine's
put-back of a declined plan (a vector regression's within rounding: see ``_same``).
"""
import pytest
import torch
from torch.distributions import Binomial, Categorical, Normal, Poisson

import mininf_amd as mi
from mininf_amd import particles
# put_back: what a planner does with a predictor its kernel cannot take
from mininf_amd.linear import DeferredMatmul, put_back

K, N, P, G, C = 4, 5, 3, 3, 3
EPS = 2.0 ** -23   # float32: the spacing of the numbers in [1, 2)
_gen = torch.Generator().manual_seed(7)
X = torch.randn(N, P, generator=_gen)
GROUP = torch.tensor([2, 0, 1, 1, 2])
STATES = {"theta": torch.randn(K, P, generator=_gen), "Theta": torch.randn(K, P, C, generator=_gen),
          "alpha": torch.randn(K, G, generator=_gen), "b": torch.rand(K, generator=_gen) + 0.5}
REAL = torch.randn(N, generator=_gen)
COUNT = torch.tensor([0., 3., 1., 2., 5.])
LABEL = torch.tensor([0, 2, 1, 1, 0])
TRIALS = torch.tensor([6, 7, 8, 9, 10])   # an observed integer total_count: cast with type_as


@pytest.fixture(autouse=True)
def host_deferral(monkeypatch):
    monkeypatch.setattr(DeferredMatmul, "require_device", False)


def _traces(sites, monkeypatch, **data):
    """The sites by name of the model ``sites(theta, Theta, alpha, b)``, traced with both
    deferrals on and with both off."""
    def model():
        theta = mi.sample("theta", Normal(0, 1), sample_shape=(P,))
        Theta = mi.sample("Theta", Normal(0, 1), sample_shape=(P, C))
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        b = mi.sample("b", Normal(0, 1))
        for name, distribution in sites(theta, Theta, alpha, b).items():
            mi.sample(name, distribution)
    out = []
    for on in (True, False):
        monkeypatch.setenv("MININF_AMD_DEFER_GATHER", "1" if on else "0")
        trace = particles.trace_particles(mi.condition(model, **data), dict(STATES), K,
                                          defer_matmul=on)
        out.append({s.name: s for s in trace.sites if s.name in data})
    return out


def _same(on, off, linear=None, gathered=None):
    """The deferred trace's site against the plain one: ``linear`` the link of a site expected to
    stay linear, ``gathered`` the links per role of one expected to stay gathered."""
    assert off.linear_X is None and off.gather_roles is None
    assert on.family == off.family
    assert (on.linear_X is not None) == (linear is not None)
    if linear is not None:
        assert on.linear_X is X and on.linear_link == linear
    assert (on.gather_roles is not None) == (gathered is not None)
    if gathered is not None:
        assert [None if g is None else g.link for g in on.gather_roles] == gathered
    theta, role = on.linear_theta, on.linear_role
    if linear is not None or gathered is not None:
        put_back(on, K)
        assert on.linear_X is None and on.gather_roles is None
    assert len(on.tensors) == len(off.tensors)
    for r, (got, want) in enumerate(zip(on.tensors, off.tensors)):
        if linear is not None and r == role:
            # The put-back of a vector regression is `theta @ X.t()`, one [K, P] x [P, N] product,
            # where the model computed `X @ theta` per particle: the same P products summed by
            # another kernel. It is pinned exactly, and held to the plain trace within the rounding
            # of two P-term float32 dot products, 2 * gamma_P * |X| @ |theta| (through exp: that
            # relative change of the result, and an ulp for each exp).
            eta = theta @ X.t()
            assert torch.equal(got, eta.exp() if linear == "exp" else eta)
            bound = P * EPS * (theta.abs() @ X.abs().t())
            if linear == "exp":
                bound = want * (torch.expm1(bound) + 2 * EPS)
            assert got.shape == want.shape and bool(((got - want).abs() <= bound).all())
            continue
        if gathered is not None and got.shape != want.shape:
            # a per-particle scalar beside a gathered role is recorded as the scalar [K]: the plain
            # trace holds its broadcast over the rows
            assert got.shape == (K,)
            got = got.reshape(K, 1).expand(K, N)
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def test_sum_of_both_materialises(monkeypatch):
    on, off = _traces(lambda th, Th, al, b: {"y": Normal(X @ th + al[GROUP], 1.)}, monkeypatch,
                      y=REAL)
    _same(on["y"], off["y"])


@pytest.mark.parametrize("swapped", [False, True])
def test_product_of_both_materialises(swapped, monkeypatch):
    def sites(th, Th, al, b):
        return {"y": Normal((X @ th) * al[GROUP] if swapped else al[GROUP] * (X @ th), 1.)}
    on, off = _traces(sites, monkeypatch, y=REAL)
    _same(on["y"], off["y"])


def test_matmul_placeholder_beside_a_gathered_role_materialises(monkeypatch):
    on, off = _traces(lambda th, Th, al, b: {"y": Normal(al[GROUP], (X @ th).exp())}, monkeypatch,
                      y=REAL)
    _same(on["y"], off["y"])


def test_a_linear_and_a_gathered_site_in_one_model(monkeypatch):
    def sites(th, Th, al, b):
        return {"y": Poisson((X @ th).exp()), "z": Poisson((b + al[GROUP]).exp())}
    on, off = _traces(sites, monkeypatch, y=COUNT, z=COUNT.flip(0))
    role = on["z"].gather_roles[0]
    assert isinstance(role.shift, torch.Tensor) and torch.equal(role.shift, STATES["b"]) and \
        role.mult is None and role.table.data_ptr() == STATES["alpha"].data_ptr()
    assert on["y"].linear_role == 0 and torch.equal(on["y"].linear_theta, STATES["theta"])
    _same(on["y"], off["y"], linear="exp")
    _same(on["z"], off["z"], gathered=["exp"])


def test_exp_of_an_exp_link_materialises(monkeypatch):
    def sites(th, Th, al, b):
        return {"y": Normal((X @ th).exp().exp(), 1.), "z": Normal(al[GROUP].exp().exp(), 1.)}
    on, off = _traces(sites, monkeypatch, y=REAL, z=REAL)
    _same(on["y"], off["y"])
    _same(on["z"], off["z"])


def test_normalisation_by_another_product_materialises(monkeypatch):
    def sites(th, Th, al, b):
        return {"y": Categorical(logits=(X @ Th) - (X @ Th).logsumexp(-1, keepdim=True))}
    on, off = _traces(sites, monkeypatch, y=LABEL)
    _same(on["y"], off["y"])


def test_broadcast_of_both_keeps_each_a_placeholder(monkeypatch):
    def sites(th, Th, al, b):
        m, g, s = torch.broadcast_tensors(X @ th, al[GROUP], b)
        return {"y": Normal(m, 1.), "z": Normal(g, s)}
    on, off = _traces(sites, monkeypatch, y=REAL, z=REAL)
    # b is recorded as the scalar per particle it came from, not as its expansion over the rows
    assert on["z"].tensors[1].shape == (K,) and torch.equal(on["z"].tensors[1], STATES["b"])
    assert off["z"].tensors[1].shape == (K, N)
    _same(on["y"], off["y"], linear="identity")
    _same(on["z"], off["z"], gathered=["identity", None])


def test_product_of_a_gather_placeholder_reads_its_values(monkeypatch):
    # `X.t() @ alpha[group]`: the gather is the product's operand, not a theta to defer
    on, off = _traces(lambda th, Th, al, b: {"y": Normal(X.t() @ al[GROUP] + 1., 1.)}, monkeypatch,
                      y=REAL[:P])
    _same(on["y"], off["y"])


def test_type_as_a_placeholder_does_not_materialise(monkeypatch):
    def sites(th, Th, al, b):
        eta, mu = X @ th, al[GROUP]
        return {"y": Binomial(TRIALS.type_as(eta), logits=eta),
                "z": Normal(mu, TRIALS.type_as(mu))}
    on, off = _traces(sites, monkeypatch, y=COUNT, z=REAL)
    assert on["y"].linear_role == 1
    _same(on["y"], off["y"], linear="identity")
    _same(on["z"], off["z"], gathered=["identity", None])
