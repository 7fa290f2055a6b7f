"""
The deferred sum ``alpha[group] + X @ theta`` on the host: with ``defer_sum=True`` the trace records
every native spelling as one gathered site with a linear term (shift, mult, link, operand order,
theta) without computing the gather or the product; everything else materialises exactly the plain
trace's values; ``put_back`` restores what the model wrote, in the model's order; and without the
keyword the trace is today's.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Normal, Poisson

import mininf_amd as mi
from mininf_amd import particles
from mininf_amd.linear import DeferredMatmul, put_back

K, G, N, P = 3, 4, 9, 5


@pytest.fixture(autouse=True)
def host_deferral(monkeypatch):
    monkeypatch.setattr(DeferredMatmul, "require_device", False)


class Spy(torch.overrides.TorchFunctionMode):
    """The gathers and products that run on a batched tensor."""
    NAMES = ("__getitem__", "index_select", "gather", "matmul", "__matmul__", "mv", "mm")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in self.NAMES and any(
                isinstance(a, torch.Tensor) and torch._C._functorch.is_batchedtensor(a)
                for a in args):
            self.seen.append(func.__name__)
        return func(*args, **(kwargs or {}))


def _inputs(p=P, n_x=N):
    torch.manual_seed(0)
    group = torch.tensor([3, 0, 1, 1, 3, 0, 0, 1, 3])
    X = torch.randn(n_x, p)
    states = {"alpha": torch.randn(K, G), "theta": 0.3 * torch.randn(K, p),
              "sigma": torch.rand(K) + 0.5, "a": torch.randn(K), "b": torch.randn(K)}
    return group, X, states


def _trace(build, data, p=P, n_x=N, **keywords):
    group, X, states = _inputs(p, n_x)

    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        theta = mi.sample("theta", Normal(0, 1), sample_shape=(p,))
        sigma = mi.sample("sigma", Normal(0, 1))
        a = mi.sample("a", Normal(0, 1))
        b = mi.sample("b", Normal(0, 1))
        mi.sample("y", build(alpha, group, X, theta, sigma, a, b))
    spy = Spy()
    with spy:
        trace = particles.trace_particles(mi.condition(model, y=data), states, K, **keywords)
    site = next(s for s in trace.sites if s.name == "y")
    return site, states, group, X, spy.seen


def _data(spelling):
    torch.manual_seed(1)
    if "poisson" in spelling:
        return torch.poisson(torch.ones(N) * 2)
    if "bernoulli" in spelling:
        return (torch.rand(N) < 0.5).float()
    return torch.randn(N)


# spelling -> (the distribution, whether the gather is the sum's left operand)
SPELLINGS = {
    "gather_first": (lambda al, g, X, th, s, a, b: Normal(al[g] + X @ th, s), True),
    "product_first": (lambda al, g, X, th, s, a, b: Normal(X @ th + al[g], s), False),
    "shifted": (lambda al, g, X, th, s, a, b: Normal(a + al[g] + X @ th, s), True),
    "affine": (lambda al, g, X, th, s, a, b: Normal((a + b * al[g]) + X @ th, s), True),
    "shift_after": (lambda al, g, X, th, s, a, b: Normal((al[g] + X @ th) + a, s), True),
    "minus_after": (lambda al, g, X, th, s, a, b: Normal((al[g] + X @ th) - 1.5, s), True),
    "poisson": (lambda al, g, X, th, s, a, b: Poisson((a + al[g] + X @ th).exp()), True),
    "poisson_torch_exp": (lambda al, g, X, th, s, a, b: Poisson(torch.exp(X @ th + al[g])), False),
    "bernoulli": (lambda al, g, X, th, s, a, b: Bernoulli(logits=X @ th + al[g]), False),
    "torch_add": (lambda al, g, X, th, s, a, b: Normal(torch.add(al[g], X @ th), s), True),
    "method_add": (lambda al, g, X, th, s, a, b: Normal((X @ th).add(al[g]), s), False),
    "radd": (lambda al, g, X, th, s, a, b: Normal(1.5 + (al[g] + X @ th), s), True),
    "mv": (lambda al, g, X, th, s, a, b: Normal(al[g] + torch.mv(X, th), s), True),
}


def _role_name(spelling):
    return "rate" if "poisson" in spelling else "logits" if "bernoulli" in spelling else "loc"


def _model_values(build, states, group, X, name):
    """The model's own spelling, particle by particle."""
    return torch.stack([getattr(build(states["alpha"][k], group, X, states["theta"][k],
                                      states["sigma"][k], states["a"][k], states["b"][k]), name)
                        for k in range(K)])


@pytest.mark.parametrize("spelling", list(SPELLINGS))
def test_native_spellings_are_recorded_without_gather_or_product(spelling):
    build, left = SPELLINGS[spelling]
    site, states, group, X, seen = _trace(build, _data(spelling), defer_sum=True)
    assert seen == [], seen
    assert site.linear_X is None          # (plan_linear, claim_linear_draws and _rows pass it by)
    roles = [g for g in site.gather_roles if g is not None]
    assert len(roles) == 1 and site.gather_roles[0] is roles[0]
    role = roles[0]
    assert role.table.data_ptr() == states["alpha"].data_ptr() and role.table.shape == (K, G)
    assert role.linear_X is X and role.linear_left is left
    assert role.linear_theta.data_ptr() == states["theta"].data_ptr()
    assert role.linear_theta.shape == (K, P)
    assert role.link == ("exp" if "poisson" in spelling else "identity")
    a, b = states["a"], states["b"]
    want_shift = {"shifted": a, "affine": a, "shift_after": a, "poisson": a}.get(spelling)
    if want_shift is not None:
        assert torch.equal(role.shift.reshape(K), want_shift)
    elif spelling in ("minus_after", "radd"):
        assert role.shift == (-1.5 if spelling == "minus_after" else 1.5)
    else:
        assert role.shift is None
    if spelling == "affine":
        assert torch.equal(role.mult.reshape(K), b)
    else:
        assert role.mult is None
    assert len(role.post) == (1 if spelling in ("shift_after", "minus_after", "radd") else 0)
    # the predictor the record stands for is the one the model wrote
    eta = states["alpha"][:, role.index.long()]
    if role.mult is not None:
        eta = role.mult.reshape(K, 1) * eta
    if role.shift is not None:
        eta = (role.shift.reshape(K, 1) if isinstance(role.shift, torch.Tensor) else role.shift) + eta
    eta = eta + role.linear_theta @ role.linear_X.t()
    got = eta.exp() if role.link == "exp" else eta
    want = _model_values(build, states, group, X, _role_name(spelling))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    assert site.tensors[1].shape == (K,) or "poisson" in spelling or "bernoulli" in spelling


@pytest.mark.parametrize("spelling", list(SPELLINGS))
def test_put_back_restores_what_the_model_wrote(spelling):
    build, _ = SPELLINGS[spelling]
    site, states, group, X, _ = _trace(build, _data(spelling), defer_sum=True)
    put_back(site, K)
    assert site.gather_roles is None
    # the model's spelling with the product as put_back spells a vector regression, bit for bit
    product = states["theta"] @ X.t()
    al = states["alpha"][:, group]
    a, b = states["a"].reshape(K, 1), states["b"].reshape(K, 1)
    want = {
        "gather_first": lambda: al + product, "product_first": lambda: product + al,
        "shifted": lambda: a + al + product, "affine": lambda: (a + b * al) + product,
        "shift_after": lambda: (al + product) + a, "minus_after": lambda: (al + product) - 1.5,
        "poisson": lambda: (a + al + product).exp(),
        "poisson_torch_exp": lambda: torch.exp(product + al),
        "bernoulli": lambda: product + al, "torch_add": lambda: al + product,
        "method_add": lambda: product + al, "radd": lambda: 1.5 + (al + product),
        "mv": lambda: al + product}[spelling]()
    assert torch.equal(site.tensors[0], want)
    # and within the vector regression's bound, plus one rounding of the sum, of the plain trace
    plain, *_ = _trace(build, _data(spelling))
    scale = (states["theta"].abs() @ X.abs().t()) + al.abs() + 1.0
    if "poisson" in spelling:
        scale = scale * plain.tensors[0].abs()
    bound = (P + 2) * 2.0 ** -23 * scale
    assert bool(((site.tensors[0] - plain.tensors[0].expand(K, N)).abs() <= bound).all())


OTHERS = {
    "mul_after": lambda al, g, X, th, s, a, b: Normal((al[g] + X @ th) * b, s),
    "number_mul_after": lambda al, g, X, th, s, a, b: Normal(2.0 * (al[g] + X @ th), s),
    "rsub_after": lambda al, g, X, th, s, a, b: Normal(1.0 - (al[g] + X @ th), s),
    "tensor_rsub_after": lambda al, g, X, th, s, a, b: Normal(a - (al[g] + X @ th), s),
    "two_gathers": lambda al, g, X, th, s, a, b: Normal(al[g] + al[g.flip(0)] + X @ th, s),
    "two_products": lambda al, g, X, th, s, a, b: Normal(al[g] + X @ th + X @ th, s),
    "exp_then_sum": lambda al, g, X, th, s, a, b: Normal(al[g].exp() + X @ th, s),
    "gathered_scale": lambda al, g, X, th, s, a, b: Normal(al[g] + X @ th, al[g].exp()),
    "sub": lambda al, g, X, th, s, a, b: Normal(al[g] - X @ th, s),
}


def _assert_same_as_plain(build, data, **shape):
    site, states, group, X, _ = _trace(build, data, defer_sum=True, **shape)
    plain, *_ = _trace(build, data, **shape)
    assert site.gather_roles is None and plain.gather_roles is None
    assert site.linear_X is None and plain.linear_X is None
    assert len(site.tensors) == len(plain.tensors)
    for got, want in zip(site.tensors, plain.tensors):
        assert got.shape == want.shape and torch.equal(got, want)
    return site, states, group, X


@pytest.mark.parametrize("spelling", list(OTHERS))
def test_everything_else_materialises_like_the_plain_trace(spelling):
    build = OTHERS[spelling]
    site, states, group, X = _assert_same_as_plain(build, _data(spelling))
    want = _model_values(build, states, group, X, "loc")
    torch.testing.assert_close(site.tensors[0].expand(K, N), want, rtol=1e-5, atol=1e-5)


def test_wide_product_materialises():
    _assert_same_as_plain(SPELLINGS["gather_first"][0], _data("normal"), p=33)


def test_matrix_theta_materialises():
    torch.manual_seed(0)
    group = torch.tensor([3, 0, 1, 1, 3, 0, 0, 1, 3])
    X = torch.randn(N, P)
    states = {"alpha": torch.randn(K, G), "Theta": 0.3 * torch.randn(K, P, 2)}
    y = torch.randn(N, 2)

    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        Theta = mi.sample("Theta", Normal(0, 1), sample_shape=(P, 2))
        mi.sample("y", Normal(alpha[group][:, None] + X @ Theta, 1.0))
    traces = [particles.trace_particles(mi.condition(model, y=y), states, K, **kw)
              for kw in ({"defer_sum": True}, {})]
    sites = [next(s for s in t.sites if s.name == "y") for t in traces]
    assert sites[0].gather_roles is None and sites[0].linear_X is None
    assert torch.equal(sites[0].tensors[0], sites[1].tensors[0])


def test_different_lengths_materialise():
    """X with one row: torch broadcasts the [1] product against the [N] gather."""
    _assert_same_as_plain(SPELLINGS["gather_first"][0], _data("normal"), n_x=1)


@pytest.mark.parametrize("spelling", ["gather_first", "product_first", "poisson"])
def test_without_the_keyword_the_trace_is_todays(spelling):
    build, _ = SPELLINGS[spelling]
    site, states, group, X, seen = _trace(build, _data(spelling))
    off, *_ = _trace(build, _data(spelling), defer_sum=False)
    for s in (site, off):
        assert s.gather_roles is None and s.linear_X is None
    assert torch.equal(site.tensors[0], off.tensors[0])
    want = _model_values(build, states, group, X, _role_name(spelling))
    torch.testing.assert_close(site.tensors[0].expand(K, N), want, rtol=1e-5, atol=1e-5)


def test_the_sum_needs_both_deferrals(monkeypatch):
    monkeypatch.setenv("MININF_AMD_DEFER_GATHER", "0")
    site, *_ = _trace(SPELLINGS["gather_first"][0], _data("normal"), defer_sum=True)
    assert site.gather_roles is None
    monkeypatch.delenv("MININF_AMD_DEFER_GATHER")
    mode = DeferredMatmul(K, defer_matmul=False, defer_gather=True, defer_sum=True)
    assert mode.defer_sum is False
    assert DeferredMatmul(K).defer_sum is False and DeferredMatmul(K, defer_sum=True).defer_sum


def test_switch_is_registered_default_on():
    from mininf_amd import switches
    assert switches.SWITCHES["DEFER_SUM"][0] is True and switches.enabled("DEFER_SUM")
