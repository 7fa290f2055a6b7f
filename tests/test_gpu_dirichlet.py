"""
Native Dirichlet on the MI355X: site density (mi_dirichlet_forward), guide factor
(mi_dirichlet_rsample and its backward) and entropy (mi_dirichlet_entropy), at kernel level and
through EvidenceLowerBoundLoss. The yardstick is torch float64 on the CPU from the same float32
inputs (tests/dirichlet_reference.py).

Tolerances: the table tolerances of DESIGN.md 0c for the density (values rtol 1e-5 / atol 2e-6,
gradients 2e-5 / 2e-5), the Beta sampler's backward bounds for the sampler's backward (rtol 1e-4 /
atol 1e-5), 1e-5 relative for the entropy and the losses, 2e-5 of the max-norm for the guide
gradients. For the density, the sampler's backward and the losses, where torch's own float32 CPU
result misses a bound on the same inputs, that bound becomes twice torch float32's error (printed;
DESIGN.md 0d records the measured figures: none needed it). The entropy bounds stand as they are.
"""
import functools

import numpy as np
import pytest
import torch
from torch.distributions import Beta, Categorical, Dirichlet, Gamma

import mininf_amd as mi
from mininf_amd import _native as nat, engine, guide
from mininf_amd.graph import StepGraph
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution
from mininf_amd.particles import SiteRecord
from tests import dirichlet_reference as ref
from tests.test_gpu_kernels import launch

pytestmark = pytest.mark.gpu

CS, NS, KS = [1, 2, 3, 63, 64, 65, 257, 1024], [1, 5], [1, 7, 64]
CHOICES = torch.tensor([0.3, 1.0, 2.5, 40.0])
VALUE_RTOL, VALUE_ATOL, GRAD_RTOL, GRAD_ATOL = 1e-5, 2e-6, 2e-5, 2e-5
BWD_RTOL, BWD_ATOL = 1e-4, 1e-5   # tests/test_gpu_kernels.py, test_beta_guide_backward_against_oracle


def concentrations(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return CHOICES[torch.randint(0, 4, shape, generator=gen)]


def excess(got, want, rtol, atol):
    """max over entries of |got - want| / (atol + rtol |want|): <= 1 passes assert_allclose."""
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    ratio = err / (atol + rtol * want.abs())
    ratio[err == 0] = 0.0   # (an exact zero against an exact zero at atol = 0)
    return float(ratio.max())


def check(what, got, want, rtol, atol, torch32=None):
    """assert_allclose at (rtol, atol); where torch's float32 result misses that bound, at twice
    torch float32's error."""
    mine = excess(got, want, rtol, atol)
    theirs = 0.0 if torch32 is None else excess(torch32, want, rtol, atol)
    factor = 1.0 if theirs <= 1.0 else 2.0 * theirs
    print(f"{what}: kernel error {mine:.3g} of the bound (rtol {rtol:g}, atol {atol:g}), "
          f"torch float32 {theirs:.3g}, allowed {factor:.3g}")
    assert mine <= factor, (what, mine, theirs)


def site(scale=1.0):
    return SiteRecord("s", "dirichlet", [], torch.Size([]), scale, None, "Dirichlet")


@functools.lru_cache(maxsize=None)
def density_case(C, N, K):
    """Concentration (per particle for N = 1, particle-constant for N = 5), simplex values, a
    masked row for N = 5, and the float64 reference (computed once per shape)."""
    torch.manual_seed(1000 * C + 10 * N + K)
    conc = concentrations((N, C), C + N) if N > 1 else concentrations((K, N, C), C + K)
    if C > 1:
        conc[..., -1] = 1.0   # every row has an a_c = 1 (xlogy's special case)
    full = conc.expand(K, N, C)
    x = Dirichlet(full.double()).sample().clamp_min(1e-30).float()
    mask = None
    if N > 1:
        mask = torch.ones(N, dtype=torch.bool)
        mask[2] = False
    scale, g0 = 2.5, -1.0 / K
    want = ref.density(full, x, None if mask is None else mask.expand(K, N), scale, g0)
    # torch's own float32 evaluation of the same thing
    a32, x32 = full.clone().requires_grad_(), x.clone().requires_grad_()
    lp32 = Dirichlet(a32, validate_args=False).log_prob(x32)
    if mask is not None:
        lp32 = torch.where(mask.expand(K, N), lp32, torch.zeros(()))
    total32 = lp32.sum(-1) * scale
    da32, dx32 = torch.autograd.grad(total32.sum() * g0, [a32, x32])
    return conc, x, mask, scale, g0, want, (total32.detach(), da32, dx32)


def run_density(device, conc, x, mask, scale, g0, K, N, C, need=(True, True)):
    a = conc.to(device).expand(K, N, C).requires_grad_(need[0])
    v = x.to(device).requires_grad_(need[1])
    m = None if mask is None else mask.to(device).reshape(1, N).expand(K, N)
    total, da, dx, flags = engine._run_dirichlet(site(scale), g0, a, v, m, need)
    torch.cuda.synchronize()
    return total, da, dx, int(flags.cpu()[0])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_density_against_float64(device, C, N, K):
    conc, x, mask, scale, g0, (want, want_da, want_dx), (t32, da32, dx32) = density_case(C, N, K)
    total, da, dx, flags = run_density(device, conc, x, mask, scale, g0, K, N, C)
    assert flags == 0
    check("total", total, want, VALUE_RTOL, VALUE_ATOL, t32)
    check("dconcentration", da, want_da, GRAD_RTOL, GRAD_ATOL, da32)
    check("dvalue", dx, want_dx, GRAD_RTOL, GRAD_ATOL, dx32)
    if mask is not None:
        assert (da[:, 2] == 0).all() and (dx[:, 2] == 0).all()
    # only the requested gradient is written
    _, none_a, only_x, _ = run_density(device, conc, x, mask, scale, g0, K, N, C, (False, True))
    assert none_a is None and torch.equal(only_x, dx)


@pytest.mark.parametrize("K", [1, 7])
def test_density_at_two_categories_is_the_beta_site(device, K):
    N = 5
    conc, x, _, _, _, _, _ = density_case(2, N, K)
    a = conc.to(device).expand(K, N, 2)
    v = x.to(device)
    total, da, dx, flags = run_density(device, conc, x, None, 1.0, -1.0, K, N, 2)
    roles = [a[..., 0].contiguous().requires_grad_(), a[..., 1].contiguous().requires_grad_()]
    # the Beta site at x with the complement 1 - x it forms itself
    btotal, bgrads, _, bflags, _ = launch("beta", roles,
                                          v[..., 0].contiguous().requires_grad_(), device, K=K, N=N)
    assert flags == 0 and int(bflags.max()) == 0
    np.testing.assert_allclose(total.cpu().numpy(), btotal.numpy(), rtol=VALUE_RTOL,
                               atol=VALUE_ATOL)
    for j in range(2):
        np.testing.assert_allclose(da[..., j].cpu().numpy(), bgrads[j].cpu().numpy(),
                                   rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # the Beta site's value gradient is d/dx_0 - d/dx_1 of the Dirichlet's (x_1 = 1 - x_0)
    np.testing.assert_allclose((dx[..., 0] - dx[..., 1]).cpu().numpy(), bgrads[2].cpu().numpy(),
                               rtol=GRAD_RTOL, atol=GRAD_ATOL)


def test_density_validation_flags(device):
    K, N, C = 3, 4, 5
    conc = torch.full((N, C), 2.0)
    x = torch.full((K, N, C), 1.0 / C)
    mask = torch.tensor([True, True, False, True])

    def flags(conc=conc, x=x, mask=None):
        return run_density(device, conc, x, mask, 1.0, -1.0, K, N, C)[3]

    assert flags() == 0
    for bad in (0.0, float("nan"), -1.0):
        c = conc.clone()
        c[1, 3] = bad
        assert flags(conc=c) & nat.FLAG_PARAM
    negative = x.clone()
    negative[1, 0, 0], negative[1, 0, 1] = -0.1, 0.5
    assert flags(x=negative) == nat.FLAG_SUPPORT
    off = x.clone()
    off[2, 3, 0] += 3e-6
    assert flags(x=off) == nat.FLAG_SUPPORT
    close = x.clone()
    close[2, 3, 0] += 2e-7   # within torch's 1e-6
    assert flags(x=close) == 0
    nan = x.clone()
    nan[0, 1, 2] = float("nan")
    assert flags(x=nan) == nat.FLAG_SUPPORT
    # the same bad rows masked out raise nothing
    bad = x.clone()
    bad[:, 2, 0] = -1.0
    c = conc.clone()
    c[2, 1] = 0.0
    assert flags(conc=c, x=bad, mask=mask) == 0


# ---- guide draws ---------------------------------------------------------------------------------
def gamma_variates(device, conc, K, seed, step, stream_id, offset):
    """mi_gamma_rsample's standard draws for the flattened concentrations at rate 1."""
    flat = conc.reshape(-1).contiguous()
    M = flat.numel()
    rate = torch.ones(1, device=device)
    g = torch.empty((K, M), device=device)
    x = torch.empty((K, M), device=device)
    nat.check(nat.lib().mi_gamma_rsample(flat.data_ptr(), 1, rate.data_ptr(), 0, K, M, seed, step,
                                         None, stream_id, offset, None, g.data_ptr(),
                                         x.data_ptr(), nat.stream_handle(device)),
              "mi_gamma_rsample")
    return g.reshape((K,) + tuple(conc.shape))


def draw(device, conc, K, seed=5, step=2, stream_id=3, offset=0, noise=None):
    cfg = guide.DrawConfig(K=K, seed=seed, step=step, stream_id=stream_id, particle_offset=offset,
                           noise=noise)
    return guide.draw(Dirichlet(conc, validate_args=False), cfg)


def support_flags(device, conc, x):
    K, N, C = x.shape
    a = conc.expand(K, N, C)
    return int(engine._run_dirichlet(site(), -1.0, a, x, None, (False, False))[3].cpu()[0])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_draw_is_the_normalised_gamma_draw(device, C, N, K):
    conc = concentrations((N, C), 7 * C + N).to(device)
    x = draw(device, conc, K)
    assert x.shape == (K, N, C) and guide.native_dirichlet(Dirichlet(conc))
    g = gamma_variates(device, conc, K, 5, 2, 3, 0)
    want = ref.normalise(g.cpu())
    torch.testing.assert_close(x.cpu().double(), want, rtol=2e-7, atol=0)
    # injected variates
    again = draw(device, conc, K, seed=99, noise=g.clone())
    torch.testing.assert_close(again.cpu().double(), want, rtol=2e-7, atol=0)
    assert support_flags(device, conc, x) == 0
    assert float(x.min()) >= ref.FLT_MIN and float(x.max()) <= ref.ONE_BELOW
    other = draw(device, conc, K, step=3)
    assert C == 1 or not torch.equal(other, x)


def test_draw_offset_invariance_and_underflow(device):
    for C in (3, 65, 1024):
        conc = concentrations((5, C), C).to(device)
        whole = draw(device, conc, 10)
        part = draw(device, conc, 7, offset=3)
        assert torch.equal(part, whole[3:])
    # every variate underflows: the clamped one-hot of the largest concentration
    conc = torch.tensor([[0.5, 2.0, 1.0], [3.0, 0.1, 0.2]], device=device)
    x = draw(device, conc, 2, noise=torch.zeros(2, 2, 3, device=device))
    want = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]).clamp(ref.FLT_MIN, ref.ONE_BELOW)
    assert torch.equal(x.cpu(), want.float().expand(2, 2, 3))
    assert support_flags(device, conc, x) == 0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_draw_backward_against_float64(device, C, N, K):
    gen = torch.Generator().manual_seed(C + 31 * N + K)
    conc = concentrations((N, C), 3 * C + N)
    g = torch.distributions.Gamma(conc.double(), 1.0).sample((K,)).clamp_min(1e-30).float()
    weights = torch.randn(K, N, C, generator=gen)
    leaf = conc.to(device).requires_grad_()
    x = draw(device, leaf, K, noise=g.to(device))
    (x * weights.to(device)).sum().backward()
    first = leaf.grad.clone()
    # float64 reference from the float32 draws the kernel saved
    a64 = conc.double().requires_grad_()
    (ref.injected_draw(a64, x.detach().cpu().double()) * weights.double()).sum().backward()
    a32 = conc.clone().requires_grad_()
    (ref.injected_draw(a32, x.detach().cpu()) * weights).sum().backward()
    check("dconcentration", first, a64.grad, BWD_RTOL, BWD_ATOL, a32.grad)
    # a second launch agrees bit for bit
    leaf.grad = None
    y = draw(device, leaf, K, noise=g.to(device))
    (y * weights.to(device)).sum().backward()
    assert torch.equal(leaf.grad, first)


# ---- entropy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_entropy_against_float64(device, C, N):
    conc = concentrations((N, C), 11 * C + N)
    leaf = conc.to(device).requires_grad_()
    h = guide.dirichlet_entropy(Dirichlet(leaf, validate_args=False))
    h.backward()
    a64 = conc.double().requires_grad_()
    want = Dirichlet(a64).entropy().sum()
    want.backward()
    a32 = conc.clone().requires_grad_()
    h32 = Dirichlet(a32).entropy().sum()
    h32.backward()
    if C > 1:
        # 1e-5 relative as it stands: torch float32's own error is printed, never allowed for
        for what, got, w64, w32 in (("entropy", h.detach().reshape(1), want.detach().reshape(1),
                                     h32.detach().reshape(1)),
                                    ("dentropy", leaf.grad, a64.grad, a32.grad)):
            print(f"{what}: torch float32 at {excess(w32, w64, 1e-5, 0.0):.3g} of the bound")
            check(what, got, w64, 1e-5, 0.0)
    else:   # a point mass: H = 0 and dH/da = (a - 1) psi'(a) - (a - 1) psi'(a) = 0 exactly
        assert abs(float(want.detach())) <= 1e-12 and float(a64.grad.abs().max()) <= 1e-12
        assert abs(float(h.detach())) <= 1e-6 and float(leaf.grad.abs().max()) <= 1e-6


def test_entropy_at_two_categories_is_the_beta_entropy(device):
    conc = concentrations((5, 2), 4)
    h = guide.dirichlet_entropy(Dirichlet(conc.to(device)))
    want = Beta(conc[:, 0].double(), conc[:, 1].double()).entropy().sum()
    assert abs(float(h) - float(want)) <= 1e-5 * abs(float(want))


# ---- through the loss ----------------------------------------------------------------------------
PRIOR_A = torch.tensor([1.0, 2.0, 0.7, 3.0, 1.5])
GUIDE_A = torch.tensor([2.0, 3.0, 1.5, 4.0, 2.5])
LABELS = torch.randint(0, 5, (37,), generator=torch.Generator().manual_seed(8))


def model_a(device, cast=False):
    """pi ~ Dirichlet(prior), z ~ Categorical(probs=pi) with 37 observed labels. ``cast``: hand the
    Categorical site float32 probabilities (its kernel takes nothing else) under a float64 guide."""
    prior, labels = PRIOR_A.to(device), LABELS.to(device)

    def model():
        pi = mi.sample("pi", Dirichlet(prior))
        mi.sample("z", Categorical(probs=pi.float() if cast else pi), sample_shape=[37])

    return mi.condition(model, z=labels)


def guide_a(device, dtype=torch.float32):
    return ParameterizedDistribution(Dirichlet, concentration=GUIDE_A.to(dtype)).to(device)


def noise_a(K, seed=0):
    torch.manual_seed(seed)
    return Gamma(GUIDE_A.double(), 1.0).sample((K,)).float()


def reference_a(u, g, float32=False):
    """Float64 (or torch float32) ELBO of model (a) and its gradient in the guide's parameter."""
    dtype = torch.float32 if float32 else torch.float64
    u = u.detach().cpu().to(dtype).clone().requires_grad_()
    conc = u.exp()
    x = ref.normalise(g).to(dtype)
    pi = ref.injected_draw(conc, x)
    lp = Dirichlet(PRIOR_A.to(dtype), validate_args=False).log_prob(pi) + \
        (pi / pi.sum(-1, keepdim=True)).log()[:, LABELS].sum(-1)
    loss = -lp.mean() - Dirichlet(conc).entropy().sum()
    loss.backward()
    return loss.detach(), u.grad


def compare_loss(loss, grads, want, want32):
    err = abs(float(loss) - float(want[0])) / abs(float(want[0]))
    err32 = abs(float(want32[0]) - float(want[0])) / abs(float(want[0]))
    bound = 1e-5 if err32 <= 1e-5 else 2 * err32
    print(f"loss {float(loss):.8g} reference {float(want[0]):.8g}: error {err:.3g}, torch float32 "
          f"{err32:.3g}, bound {bound:.3g}")
    assert err <= bound
    for name, got in grads.items():
        w, w32 = want[1][name], want32[1][name]
        scale = float(w.abs().max())
        e = float((got.cpu().double() - w).abs().max()) / scale
        e32 = float((w32.double() - w).abs().max()) / scale
        b = 2e-5 if e32 <= 2e-5 else 2 * e32
        print(f"  d{name}: error {e:.3g} of the max-norm, torch float32 {e32:.3g}, bound {b:.3g}")
        assert e <= b, name


@pytest.mark.parametrize("K", [8, 40])
def test_model_a_against_float64(device, K):
    module = guide_a(device)
    g = noise_a(K)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=3)
    loss = loss_fn(model_a(device), {"pi": module()}, _noise={"pi": g.to(device)})
    loss.backward()
    assert loss_fn.last_fusions["dirichlet_draws"] == 1
    u = module.distribution_parameters["concentration"]
    want, want32 = reference_a(u, g), reference_a(u, g, float32=True)
    compare_loss(loss.detach(), {"concentration": u.grad},
                 (want[0], {"concentration": want[1]}), (want32[0], {"concentration": want32[1]}))


@functools.lru_cache(maxsize=None)
def data_b():
    torch.manual_seed(12)
    y = Dirichlet(torch.tensor([2.0, 1.0, 3.0, 0.5]).double()).sample((12,)).clamp_min(1e-6)
    return (y / y.sum(-1, keepdim=True)).float()


def model_b(device):
    y = data_b().to(device)
    two, one = torch.tensor(2.0, device=device), torch.tensor(1.0, device=device)

    def model():
        a = mi.sample("a", Gamma(two, one), sample_shape=[4])
        with mi.batch(100):
            mi.sample("y", Dirichlet(a), sample_shape=[12])

    return mi.condition(model, y=y)


def reference_b(params, g, float32=False, rows=None, scale=100.0 / 12.0):
    dtype = torch.float32 if float32 else torch.float64
    leaves = {n: p.detach().cpu().to(dtype).clone().requires_grad_() for n, p in params.items()}
    conc, rate = leaves["concentration"].exp(), leaves["rate"].exp()
    a = ref.injected_gamma(conc, rate, g.to(dtype))
    y = data_b().to(dtype)
    if rows is not None:   # only the observed rows count
        y = y[rows]
    lp = Gamma(torch.tensor(2.0, dtype=dtype), torch.tensor(1.0, dtype=dtype)).log_prob(a).sum(-1) \
        + scale * Dirichlet(a[:, None, :], validate_args=False).log_prob(y).sum(-1)
    loss = -lp.mean() - Gamma(conc, rate).entropy().sum()
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in leaves.items()}


@pytest.mark.parametrize("K", [8, 40])
def test_model_b_against_float64(device, K):
    module = ParameterizedDistribution(Gamma, concentration=torch.tensor([3.0, 2.0, 4.0, 1.5]),
                                       rate=torch.tensor([1.5, 2.0, 1.2, 2.5])).to(device)
    torch.manual_seed(K)
    g = Gamma(torch.tensor([3.0, 2.0, 4.0, 1.5]).double(), 1.0).sample((K,)).float()
    seen = []
    original = engine.plan_groups

    def spy(trace, *args, **kwargs):
        seen.append(([s.family for s in trace.sites], [s.scale for s in trace.sites],
                     list(trace.fallback)))
        return original(trace, *args, **kwargs)

    engine.plan_groups = spy
    try:
        loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=3)
        loss = loss_fn(model_b(device), {"a": module()}, _noise={"a": g.to(device)})
        loss.backward()
    finally:
        engine.plan_groups = original
    families, scales, fallback = seen[-1]
    assert families == ["gamma", "dirichlet"] and fallback == []
    assert scales[1] == pytest.approx(100.0 / 12.0)
    params = dict(module.distribution_parameters.items())
    want, want32 = reference_b(params, g), reference_b(params, g, float32=True)
    compare_loss(loss.detach(), {n: p.grad for n, p in params.items()}, want, want32)


def test_masked_rows_through_the_loss(device):
    """A MaskedTensor observation: a row counts when all its categories are observed; the masked
    rows (here outside the simplex, and one with a NaN) add nothing and raise nothing."""
    K = 8
    y = data_b().clone()
    rows = torch.ones(12, dtype=torch.bool)
    rows[3] = rows[7] = False
    y[3] = torch.tensor([0.5, 0.7, -0.1, 0.2])
    y[7, 1] = float("nan")
    mask = rows[:, None].expand(12, 4).contiguous()
    two, one = torch.tensor(2.0, device=device), torch.tensor(1.0, device=device)

    def model():
        a = mi.sample("a", Gamma(two, one), sample_shape=[4])
        mi.sample("y", Dirichlet(a), sample_shape=[12])

    module = ParameterizedDistribution(Gamma, concentration=torch.tensor([3.0, 2.0, 4.0, 1.5]),
                                       rate=torch.tensor([1.5, 2.0, 1.2, 2.5])).to(device)
    torch.manual_seed(5)
    g = Gamma(torch.tensor([3.0, 2.0, 4.0, 1.5]).double(), 1.0).sample((K,)).float()
    observed = torch.masked.as_masked_tensor(y.to(device), mask.to(device))
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=3)
    loss = loss_fn(mi.condition(model, y=observed), {"a": module()}, _noise={"a": g.to(device)})
    loss.backward()
    params = dict(module.distribution_parameters.items())
    want = reference_b(params, g, rows=rows, scale=1.0)
    want32 = reference_b(params, g, float32=True, rows=rows, scale=1.0)
    compare_loss(loss.detach(), {n: p.grad for n, p in params.items()}, want, want32)


def evaluate_a(device, seed, dtype=torch.float32, K=8):
    module = guide_a(device, dtype)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=seed)
    traces = []
    original = engine.plan_groups

    def spy(trace, *args, **kwargs):
        traces.append(trace)
        return original(trace, *args, **kwargs)

    engine.plan_groups = spy
    try:
        loss = loss_fn(model_a(device, cast=dtype != torch.float32), {"pi": module()})
        loss.backward()
    finally:
        engine.plan_groups = original
    torch.cuda.synchronize()
    grad = module.distribution_parameters["concentration"].grad.detach().clone()
    return loss.detach().clone(), grad, dict(loss_fn.last_fusions), traces[-1]


def test_loss_takes_the_native_path(device):
    loss, grad, fusions, trace = evaluate_a(device, seed=21)
    assert fusions["dirichlet_draws"] == 1
    assert trace.fallback == []
    assert [s.family for s in trace.sites] == ["dirichlet", "categorical"]
    assert torch.isfinite(loss) and torch.isfinite(grad).all()


def test_loss_is_governed_by_its_seed(device):
    torch.manual_seed(1)
    loss_a, grad_a, _, _ = evaluate_a(device, seed=21)
    torch.manual_seed(2)
    loss_b, grad_b, _, _ = evaluate_a(device, seed=21)
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)
    loss_c, _, _, _ = evaluate_a(device, seed=22)
    assert not torch.equal(loss_a, loss_c)


def test_float64_guide_keeps_the_torch_path(device):
    loss, grad, fusions, trace = evaluate_a(device, seed=21, dtype=torch.float64)
    assert fusions["dirichlet_draws"] == 0
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert grad.dtype == torch.float64


def test_validation_errors_in_model_order(device):
    prior = PRIOR_A.to(device)

    def model():
        mi.sample("first", Dirichlet(prior))
        mi.sample("second", Dirichlet(prior))

    good = torch.full((5,), 0.2, device=device)
    bad = torch.tensor([0.5, 0.5, 0.2, -0.2, 0.0], device=device)
    q = {"q": torch.distributions.Normal(torch.zeros((), device=device), 1.0)}
    loss_fn = EvidenceLowerBoundLoss(num_particles=4)
    with pytest.raises(ValueError, match="'first' is not in the support of Dirichlet"):
        loss_fn(mi.condition(model, first=bad, second=bad), q)
    with pytest.raises(ValueError, match="'second' is not in the support of Dirichlet"):
        loss_fn(mi.condition(model, first=good, second=bad), q)

    def bad_parameter():
        mi.sample("first", Dirichlet(mi.value("c", shape=(5,))))

    with pytest.raises(ValueError, match="distribution Dirichlet for site 'first' to satisfy"):
        loss_fn(mi.condition(bad_parameter, first=good,
                             c=torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0], device=device)), q)
    def nan_parameter():   # (the value site itself is real: the NaN arises in the model)
        mi.sample("first", Dirichlet(mi.value("c", shape=(5,)).sqrt()))

    with pytest.raises(ValueError, match="distribution Dirichlet for site 'first' to satisfy"):
        loss_fn(mi.condition(nan_parameter, first=good,
                             c=torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0], device=device)), q)
    # a parameter violation in an earlier site wins over a support violation in a later one
    def both():
        mi.sample("first", Dirichlet(mi.value("c", shape=(5,))))
        mi.sample("second", Dirichlet(prior))

    with pytest.raises(ValueError, match="distribution Dirichlet for site 'first' to satisfy"):
        loss_fn(mi.condition(both, first=good, second=bad,
                             c=torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0], device=device)), q)
    assert torch.isfinite(loss_fn(mi.condition(model, first=good, second=good), q))


def test_captured_step_draws_anew_on_every_replay(device):
    module = guide_a(device)
    optimizer = mi.optim.Adam(module.parameters(), lr=0.01)
    loss_fn = EvidenceLowerBoundLoss(num_particles=8, seed=17)
    model = model_a(device)

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(model, {"pi": module()})
        loss.backward()
        optimizer.step()
        return loss

    captured = StepGraph(step, warmup=1)
    losses = [float(captured()) for _ in range(5)]
    captured.check()
    assert loss_fn.last_fusions["dirichlet_draws"] == 1
    assert all(np.isfinite(losses)) and len(set(losses)) == 5
