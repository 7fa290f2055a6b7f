"""
The count regressions on a deferred X @ theta (Poisson with the log link, Binomial and
NegativeBinomial with logits) without a GPU: the trace records them as linear sites without
computing the product, every other spelling materialises what torch would compute, the library's
workspace size follows the fp64 geometry with nv = 1 + P, the fp64 reference of
tests/count_linear_reference.py agrees with torch.distributions, and a float32 restatement of the
kernels' formula meets the GPU file's bounds on its inputs.
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.distributions import Binomial, NegativeBinomial, Normal, Poisson

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd import particles
from mininf_amd.linear import DeferredMatmul
from tests import test_gpu_count_linear as gpu
from tests.count_linear_reference import float32_restatement, reference
from tests.linear_reference import Prior, mfma_eligible

PO, BI, NB = nat.POISSON, nat.BINOMIAL, nat.NEGATIVE_BINOMIAL


@pytest.fixture(autouse=True)
def host_deferral(monkeypatch):
    monkeypatch.setattr(DeferredMatmul, "require_device", False)


MODES = []   # the DeferredMatmul modes of the traces of a test


@pytest.fixture(autouse=True)
def record_modes(monkeypatch):
    MODES.clear()
    init = DeferredMatmul.__init__

    def spy(self, *args, **kwargs):
        init(self, *args, **kwargs)
        MODES.append(self)
    monkeypatch.setattr(DeferredMatmul, "__init__", spy)


def trace(model, K=4, p=3, seed=0):
    theta = torch.randn(K, p, generator=torch.Generator().manual_seed(seed))
    return particles.trace_particles(model, {"theta": theta}, K), theta


def products_computed():
    """The deferred products of the test's traces that something materialised."""
    infos = [info for mode in MODES for info in mode.deferred.values()]
    assert infos, "nothing was deferred"
    return [info for info in infos if info.real is not None]


X = torch.randn(50, 3, generator=torch.Generator().manual_seed(1))
COUNTS = torch.arange(50).float() % 7 + 3.0
Y = torch.arange(50).float() % 4


def likelihood(kind, eta):
    if kind == "poisson":
        return Poisson(eta.exp())
    if kind == "poisson_torch_exp":
        return Poisson(torch.exp(eta))
    if kind == "binomial":
        return Binomial(COUNTS, logits=eta)
    if kind == "binomial_constant":
        return Binomial(12, logits=eta)
    return NegativeBinomial(COUNTS / 2, logits=eta)


@pytest.mark.parametrize("kind,family,link,role", [
    ("poisson", "poisson", "exp", 0), ("poisson_torch_exp", "poisson", "exp", 0),
    ("binomial", "binomial", "identity", 1), ("binomial_constant", "binomial", "identity", 1),
    ("negative_binomial", "negative_binomial", "identity", 1)])
def test_count_regression_recorded_without_product(kind, family, link, role):
    def model():
        theta = mi.sample("theta", Normal(0.0, 1.0), sample_shape=3)
        mi.sample("y", likelihood(kind, X @ theta))

    t, theta = trace(mi.condition(model, y=Y))
    site = next(s for s in t.sites if s.name == "y")
    assert site.family == family and site.linear_X is X
    assert site.linear_link == link and site.linear_role == role
    torch.testing.assert_close(site.linear_theta, theta)
    placeholder = site.tensors[role]
    assert placeholder.shape == (4, 50) and placeholder.stride() == (0, 0)
    assert products_computed() == []     # no GEMM ran: neither the root nor a derived placeholder


def test_broadcast_keeps_the_exp_link():
    def model():
        theta = mi.sample("theta", Normal(0.0, 1.0), sample_shape=3)
        mi.sample("y", Poisson((X @ theta).exp().expand(50)))

    t, _ = trace(mi.condition(model, y=Y))
    site = next(s for s in t.sites if s.name == "y")
    assert site.linear_X is X and site.linear_link == "exp"
    assert products_computed() == []


@pytest.mark.parametrize("use", ["binomial_probs", "negative_binomial_probs", "latent_count",
                                 "rate_without_exp", "exp_of_shifted", "exp_as_logits"])
def test_other_spellings_materialise(use):
    def model():
        theta = mi.sample("theta", Normal(0.0, 1.0), sample_shape=3)
        eta = X @ theta
        if use == "binomial_probs":
            mi.sample("y", Binomial(COUNTS, probs=torch.sigmoid(eta)))
        elif use == "negative_binomial_probs":
            mi.sample("y", NegativeBinomial(COUNTS, probs=torch.sigmoid(eta)))
        elif use == "latent_count":
            mi.sample("y", NegativeBinomial(theta[0].exp() + COUNTS, logits=eta))
        elif use == "rate_without_exp":
            mi.sample("y", Poisson(eta))
        elif use == "exp_of_shifted":
            mi.sample("y", Poisson((eta + 1.0).exp()))
        else:
            mi.sample("y", Binomial(COUNTS, logits=eta.exp()))

    t, theta = trace(mi.condition(model, y=Y))
    site = next(s for s in t.sites if s.name == "y")
    assert site.linear_X is None
    assert products_computed() != []
    real = theta @ X.T
    if use in ("binomial_probs", "negative_binomial_probs"):
        cls = Binomial if use == "binomial_probs" else NegativeBinomial
        want = cls(COUNTS, probs=torch.sigmoid(real)).logits
        torch.testing.assert_close(site.tensors[1], want)
    elif use == "latent_count":
        torch.testing.assert_close(site.tensors[1], real)
        torch.testing.assert_close(site.tensors[0], theta[:, :1].exp() + COUNTS)
    elif use == "rate_without_exp":
        torch.testing.assert_close(site.tensors[0], real)
    elif use == "exp_of_shifted":
        torch.testing.assert_close(site.tensors[0], (real + 1.0).exp())
    else:
        torch.testing.assert_close(site.tensors[1], real.exp())


# ---- host geometry ----------------------------------------------------------------------------------
BASE = 0x10000   # a dummy non-null, 16-byte aligned address: nothing is dereferenced


def test_workspace_bytes_follow_the_geometry_with_one_slot_per_feature():
    assert len(gpu.ALL_CASES) > 80
    word = ctypes.c_uint32(0)
    for case, valu in gpu.ALL_CASES:
        g = case.check_variant(valu)
        L = nat.Linear()
        L.K, L.N, L.P = case.K, case.N, case.P
        L.family = case.family
        L.options = nat.LINEAR_VALU if valu else 0
        L.x, L.x_stride_i, L.x_stride_j = BASE, case.P, 1
        L.theta, L.theta_stride_k, L.theta_stride_j = BASE, case.P, 1
        L.value, L.value_stride_i = BASE, 1
        L.scale, L.scale_stride_k = BASE, 1      # ignored by these families: no dsigma slot
        L.count, L.count_stride_i = BASE, 1
        L.grad_scale, L.site_scale, L.compute_grads = -1.0, 3.0, 1
        if case.prior:
            L.prior.present, L.prior.family = 1, gpu.PRIOR.family
            L.prior.constant[0], L.prior.constant[1] = gpu.PRIOR.c0, gpu.PRIOR.c1
            L.prior.scale = gpu.PRIOR.scale
            L.prior.flags = ctypes.addressof(word)
        assert mfma_eligible(case.P, case.P, 1, BASE, valu) == g.mfma
        size = ctypes.c_size_t()
        assert nat.lib().mi_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == 0
        assert size.value == g.workspace_bytes, (case.id, valu, vars(g))


def test_struct_size_is_checked_at_load():
    size = ctypes.c_size_t()
    assert nat.lib().mi_linear_struct_size(ctypes.byref(size)) == 0
    assert size.value == ctypes.sizeof(nat.Linear)
    assert nat.Linear.count.offset > nat.Linear.stamps.offset   # appended: a zeroed tail is valid


# ---- the fp64 reference against torch.distributions ---------------------------------------------------
@pytest.mark.parametrize("family", [PO, BI, NB], ids=list(gpu.NAMES.values()))
@pytest.mark.parametrize("prior", [False, True], ids=["plain", "prior"])
def test_reference_against_torch_float64(family, prior):
    rng = np.random.default_rng(7)
    N, P, K = 50, 3, 5
    Xn = rng.normal(size=(N, P)).astype(np.float32)
    theta = (0.5 * rng.normal(size=(K, P))).astype(np.float32)
    mask = rng.random(N) > 0.2
    if family == BI:
        count = rng.integers(1, 12, size=N).astype(np.float32)
        y = rng.binomial(count.astype(np.int64), 0.4).astype(np.float32)
    else:
        count = rng.choice([0.5, 2.0, 6.0], size=N).astype(np.float32)
        y = rng.poisson(2.0, size=N).astype(np.float32)
    if family == NB:
        y[:3], count[:3] = 0.0, 0.0     # the point mass
        mask[:3] = True
    pr = Prior(nat.NORMAL, 0.3, 1.5, 0.7) if prior else None
    scale, g0 = 3.0, -0.2
    total, dtheta, _, _ = reference(family, Xn, theta, y, mask, count, scale, g0, prior=pr)

    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    eta = th @ torch.tensor(Xn, dtype=torch.float64).T
    yt, ct = torch.tensor(y, dtype=torch.float64), torch.tensor(count, dtype=torch.float64)
    if family == PO:
        d = Poisson(eta.exp())
    elif family == BI:
        d = Binomial(ct, logits=eta)
    else:
        d = NegativeBinomial(ct, logits=eta, validate_args=False)
    lp = scale * (d.log_prob(yt) * torch.tensor(mask)).sum(1)
    if prior:
        lp = lp + pr.scale * Normal(torch.tensor(pr.c0, dtype=torch.float64),
                                       torch.tensor(pr.c1, dtype=torch.float64)).log_prob(th).sum(1)
    (g0 * lp.sum()).backward()
    np.testing.assert_allclose(total, lp.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dtheta, th.grad.numpy(), rtol=1e-12, atol=1e-12)


# ---- the kernels' float32 formula on the GPU file's inputs ---------------------------------------------
# Every input set of the GPU file: the cases that differ only in how they are launched (VALU option,
# no gradients, strides) share their arrays. Of the 8161 particles of the multi-stage geometries
# every 128th is restated (the particles are independent: a column of eta each).
RESTATED = list({c.id: c for c in (
    gpu.MULTI_STAGE + gpu.ONE_STAGE + gpu.VALU_ONLY + gpu.CROSS + gpu.FOLDED + gpu.CONSTANT +
    [c for c, _ in gpu.REGIMES])}.values())


@pytest.mark.parametrize("case", RESTATED, ids=gpu.ids(RESTATED))
def test_float32_restatement_meets_the_bounds(case):
    a = gpu.inputs(case)
    g0 = -1.0 / case.K
    ks = slice(None, None, 128 if case.K > 1000 else 1)
    theta = a["theta"][ks]
    prior = gpu.PRIOR if case.prior else None
    want, dtheta, bound, tbound = reference(case.family, a["X"], theta, a["y"], a["mask"],
                                            a["count"], gpu.SITE_SCALE, g0, row_index=a["rows"],
                                            prior=prior)
    if case.regime == "plain":
        eta = a["X"].astype(np.float64) @ a["theta"].astype(np.float64).T
        assert np.abs(eta).max() <= 3.0
    total, grad = float32_restatement(case.family, a["X"], theta, a["y"], a["mask"],
                                      a["count"], gpu.SITE_SCALE, g0, row_index=a["rows"],
                                      prior=prior)
    terr = np.abs(total - want)
    print("RESTATED", case.id, (terr / (1e-5 * tbound)).max(), (terr / (1e-5 * np.abs(want))).max(),
          (np.abs(grad - dtheta) / (1e-5 * abs(g0) * bound + 1e-7)).max())
    # the GPU file's own bounds. (With eta as the float32 chain the restatement carries the kernels'
    # whole rounding but the hardware transcendentals' last ulp: at eta up to 8 the rounding of eta
    # alone, exp(eta) * ulp(8) per row, takes 0.36 of the gradient bound.)
    assert (terr <= 1e-5 * tbound).all()
    if case.regime == "plain":
        assert (terr <= 1e-5 * np.abs(want)).all()
    assert (np.abs(grad - dtheta) <= 1e-5 * abs(g0) * bound + 1e-7).all()
