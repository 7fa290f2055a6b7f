"""
The site families beyond the first eight on the MI355X: Exponential, Laplace, Cauchy, HalfNormal,
HalfCauchy, LogNormal (and the same TransformedDistribution spelled out), StudentT with a constant
df, Binomial and NegativeBinomial, evaluated by the HIP site kernels / site programs.

The yardstick is torch.distributions in float64 on the CPU, computed here from the same float32
inputs. Tolerances are the project's table tolerances (tests/test_gpu_examples.py): rtol 1e-5 /
atol 2e-6 for values, 2e-5 / 2e-5 for gradients (vectors by max-norm in the ELBO tests, as
tests/test_gpu_parity.py does). No family needs a wider bound at these inputs (DESIGN.md section
0c lists what torch's own float32 evaluation loses against float64 at the same inputs).
"""
import functools

import numpy as np
import pytest
import torch
from torch.distributions import Binomial, Cauchy, Exponential, ExpTransform, Gamma, HalfCauchy, \
    HalfNormal, Laplace, LogNormal, NegativeBinomial, Normal, StudentT, TransformedDistribution, \
    transform_to

import mininf_amd as mi
from mininf_amd import _native as nat, particles
from mininf_amd.graph import StepGraph
from mininf_amd.particles import SiteRecord
from tests import test_gpu_kernels
from tests.test_gpu_kernels import launch

pytestmark = pytest.mark.gpu

VALUE_RTOL, VALUE_ATOL = 1e-5, 2e-6
GRAD_RTOL, GRAD_ATOL = 2e-5, 2e-5

f32 = functools.partial(np.asarray, dtype=np.float32)


def grid(*axes):
    """The cartesian product of the axes, one float32 column per axis."""
    mesh = np.meshgrid(*[f32(a) for a in axes], indexing="ij")
    return [m.reshape(-1) for m in mesh]


def tables():
    """
    name -> (family, parameter columns, value column, df, torch constructor): about 24 rows per
    family that cover every branch of its formula.
    """
    out = {}
    rate, v = grid([0.1, 0.5, 1.0, 2.0, 7.5, 30.0], [0.0, 1e-3, 0.7, 12.5])
    out["exponential"] = ("exponential", [rate], v, 0.0, Exponential)
    loc, scale, d = grid([-1.5, 0.0, 2.0], [0.3, 4.0], [0.0, -1e-3, 0.5, -40.0])
    out["laplace"] = ("laplace", [loc, scale], loc + d, 0.0, Laplace)   # d = 0: v == loc
    loc, scale, y = grid([-1.5, 2.0], [0.3, 4.0], [0.0, 1e-4, -1e-2, 0.8, -30.0, 1e4])
    out["cauchy"] = ("cauchy", [loc, scale], loc + y * scale, 0.0, Cauchy)
    scale, v = grid([0.5, 1.0, 3.0, 20.0], [0.0, 1e-3, 0.5, 2.0, 5.0, 9.0])
    out["half_normal"] = ("half_normal", [scale], v, 0.0, HalfNormal)
    scale, v = grid([0.5, 1.0, 3.0, 20.0], [0.0, 1e-3, 0.5, 2.0, 50.0, 1e4])
    out["half_cauchy"] = ("half_cauchy", [scale], v, 0.0, HalfCauchy)
    loc, scale, v = grid([-0.5, 1.2], [0.4, 2.5], [1e-3, 0.5, 0.999, 1.0, 1.001, 1e3])
    out["log_normal"] = ("log_normal", [loc, scale], v, 0.0, LogNormal)
    loc, scale, y = grid([-1.5, 2.0], [0.3, 4.0], [1e-3, -0.8, 3.0, 1e3])
    for df in (1.0, 2.5, 30.0):
        out[f"student_t_{df}"] = ("student_t", [loc, scale], loc + y * scale, df,
                                  functools.partial(StudentT, df))
    # v = 0, v = n and in between; n = 0; logits +-8
    n = f32([0, 0, 0, 1, 1, 1, 1, 5, 5, 5, 5, 5, 5, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20])
    k = f32([0, 0, 0, 0, 1, 0, 1, 0, 5, 2, 3, 0, 5, 0, 20, 7, 13, 0, 20, 0, 20, 19, 1, 10])
    lg = f32([-8, 0.3, 8, -8, -8, 8, 8, -0.7, -0.7, 0, 1.3, 8, -8, -0.7, 1.3, 0, 0.3, -8, 8, 8, -8,
              8, -8, 2.5])
    out["binomial"] = ("binomial", [n, lg], k, 0.0, lambda n, l: Binomial(n, logits=l))
    # total_count + v == 0 (rows 0-2), fractional total_count, logits +-8
    r = f32([0, 0, 0, 0.5, 0.5, 0.5, 0.5, 0.5, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5, 7, 7, 7, 7, 7, 7,
             0.5, 2.5, 7, 7])
    k = f32([0, 0, 0, 0, 1, 4, 17, 0, 0, 1, 4, 17, 17, 0, 0, 1, 4, 17, 17, 0, 4, 4, 1, 4])
    lg = f32([-8, 0.9, 8, -0.6, 0.9, -8, 8, 8, -8, -0.6, 0.9, 8, -8, 8, 0.9, -0.6, 8, -8, 0.9, -8,
              8, -8, 8, -0.6])
    out["negative_binomial"] = ("negative_binomial", [r, lg], k, 0.0,
                                lambda r, l: NegativeBinomial(r, logits=l))
    return out


def reference(make, params, value):
    """log_prob and its parameter gradients from torch.distributions in float64 on the CPU."""
    leaves = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    lp = make(*leaves).log_prob(torch.tensor(value, dtype=torch.float64))
    grads = torch.autograd.grad(lp.sum(), leaves, allow_unused=True)
    return lp.detach().numpy(), [None if g is None else g.numpy() for g in grads]


def launch_site(monkeypatch, family, roles, value, device, df=0.0, **kwargs):
    """tests.test_gpu_kernels.launch for a site that carries mi_site.extra (StudentT's df)."""
    monkeypatch.setattr(test_gpu_kernels, "SiteRecord", functools.partial(SiteRecord, extra=df))
    return launch(family, roles, value, device, **kwargs)


@pytest.mark.parametrize("mode", ["particle", "dense"])
def test_new_family_tables(device, mode, monkeypatch):
    for name, (family, params, value, df, make) in tables().items():
        want_lp, want_grads = reference(make, params, value)
        assert np.isfinite(want_lp).all(), name
        n = len(value)
        K, N = (n, 1) if mode == "particle" else (1, n)
        roles = [torch.as_tensor(p, device=device).reshape(K, N).clone().requires_grad_()
                 for p in params]
        val = torch.as_tensor(value, device=device).reshape(K, N).contiguous()
        total, grads, slot_grad, flags, _ = launch_site(monkeypatch, family, roles, val, device,
                                                         df=df, K=K, N=N)
        assert (flags == 0).all(), name
        if mode == "particle":
            got_grads = [-slot_grad[j].numpy() for j in range(len(params))]
            print(name, "lp err", np.abs(total.numpy() - want_lp).max())
            np.testing.assert_allclose(total.numpy(), want_lp, rtol=VALUE_RTOL,
                                       atol=VALUE_ATOL, err_msg=name)
        else:
            got_grads = [-g.cpu().numpy()[0] for g in grads[:len(params)]]   # (then the value's)
            print(name, "sum err", abs(total.numpy()[0] - want_lp.sum()), want_lp.sum())
            np.testing.assert_allclose(total.numpy()[0], want_lp.sum(), rtol=VALUE_RTOL,
                                       atol=VALUE_ATOL, err_msg=name)
        for j, (got, want) in enumerate(zip(got_grads, want_grads)):
            if family == "binomial" and j == 0:
                # torch gives total_count no meaningful gradient: the kernel's is 0
                assert (got == 0).all(), name
                continue
            # (NegativeBinomial at total_count = 0: torch's masked lgamma(0) backward is 0 * inf)
            ok = np.isfinite(want)
            assert ok.sum() >= n - 3, name
            print(name, f"d{j} err", np.abs(got[ok] - want[ok]).max())
            np.testing.assert_allclose(got[ok], want[ok], rtol=GRAD_RTOL, atol=GRAD_ATOL,
                                       err_msg=f"{name} d{j}")


# family -> (good parameters, good value, out-of-support value, (role, bad parameter), df)
FLAG_CASES = {
    "exponential": ([1.5], 0.5, -1.0, (0, 0.0), 0.0),
    "laplace": ([0.5, 1.5], 0.5, float("nan"), (1, -1.0), 0.0),
    "cauchy": ([0.5, 1.5], 0.5, float("nan"), (1, 0.0), 0.0),
    "half_normal": ([1.5], 0.5, -0.5, (0, -2.0), 0.0),
    "half_cauchy": ([1.5], 0.5, -0.5, (0, 0.0), 0.0),
    "log_normal": ([0.5, 1.5], 0.5, 0.0, (1, -1.0), 0.0),
    "student_t": ([0.5, 1.5], 0.5, float("nan"), (1, 0.0), 4.0),
    "binomial": ([5.0, 0.5], 2.0, 6.0, (0, -1.0), 0.0),            # v > total_count
    "negative_binomial": ([2.5, 0.5], 2.0, 1.5, (0, -0.5), 0.0),   # a fractional count
}


@pytest.mark.parametrize("family", sorted(FLAG_CASES))
def test_new_family_flags(device, family, monkeypatch):
    params, good, outside, (bad_role, bad_value), df = FLAG_CASES[family]
    N = 4

    def run(values, mask, roles=None):
        roles = roles or [torch.full((1, N), p, device=device) for p in params]
        value = torch.tensor([values], device=device)
        *_, flags, _ = launch_site(monkeypatch, family, roles, value, device, df=df, K=1, N=N,
                                   mask=torch.tensor(mask, device=device))
        return int(flags.max())

    assert run([good] * N, [True] * N) == 0
    assert run([good, outside, good, good], [True] * N) == nat.FLAG_SUPPORT
    assert run([good, outside, good, good], [True, False, True, True]) == 0   # masked out
    roles = [torch.full((1, N), p, device=device) for p in params]
    roles[bad_role][0, 2] = bad_value
    # (a negative total_count also puts every count outside [0, total_count])
    assert run([good] * N, [True] * N, roles) & nat.FLAG_PARAM


def test_student_t_df_flag_and_integer_count_checks(device, monkeypatch):
    one = torch.ones(1, 4, device=device)
    *_, flags, _ = launch_site(monkeypatch, "student_t", [one, one], one, device, df=0.0, K=1, N=4)
    assert int(flags.max()) == nat.FLAG_PARAM   # df <= 0
    cases = [("binomial", [2.5 * one, one], one, nat.FLAG_PARAM),      # fractional total_count
             ("binomial", [5 * one, one], -one, nat.FLAG_SUPPORT),
             ("binomial", [5 * one, one], 1.5 * one, nat.FLAG_SUPPORT),
             ("negative_binomial", [2 * one, one], -one, nat.FLAG_SUPPORT)]
    for family, roles, value, want in cases:
        *_, flags, _ = launch_site(monkeypatch, family, roles, value, device, K=1, N=4)
        assert int(flags.max()) == want, (family, value)


# ------------------------------------------------------------------------------------------------
# Through the loss: the same ELBO from the same draws with plain torch.distributions in float64.
# ------------------------------------------------------------------------------------------------
K = 8


def close(got, want, rtol, atol, what):
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, np.float64)
    want = np.asarray(want.detach() if isinstance(want, torch.Tensor) else want, np.float64)
    err, size = np.abs(got - want).max(), np.abs(want).max()
    print(what, "err", err, "of", size)
    assert err <= rtol * size + atol, (what, err, size)


class _StandardGamma(torch.autograd.Function):
    """Injected standard Gamma draws g as a function of the concentration: the implicit
    reparameterisation gradient torch's Gamma.rsample has (torch._standard_gamma_grad)."""
    @staticmethod
    def forward(ctx, concentration, g):
        ctx.save_for_backward(concentration, g)
        return g.clone()

    @staticmethod
    def backward(ctx, grad):
        concentration, g = ctx.saved_tensors
        return (grad * torch._standard_gamma_grad(concentration.expand_as(g), g)).sum(0) \
            .reshape(concentration.shape), None


def guide_and_noise(spec, device, seed):
    """spec: name -> (Normal, loc, scale) or (Gamma, concentration, rate); `inject` noise for
    every factor (standard normals; standard Gamma draws) from a host generator."""
    gen = torch.Generator().manual_seed(seed)
    factors, noise = {}, {}
    for name, (cls, first, second) in spec.items():
        first, second = torch.as_tensor(first), torch.as_tensor(second)
        if cls is Normal:
            factors[name] = mi.nn.ParameterizedDistribution(Normal, loc=first, scale=second)
            noise[name] = torch.randn((K,) + tuple(first.shape), generator=gen)
        else:
            factors[name] = mi.nn.ParameterizedDistribution(Gamma, concentration=first,
                                                            rate=second)
            noise[name] = torch._standard_gamma(first.expand((K,) + tuple(first.shape)).clone(),
                                                generator=gen)
    return mi.nn.ParameterizedFactorizedDistribution(**factors).to(device), noise


def reference_elbo(approx, noise, log_joint):
    """
    -(1 / K) sum_k log_joint(draws_k) - sum_f entropy_f in float64 on the CPU, from float64 copies
    of the guide's unconstrained parameters; returns (loss, {factor: {parameter: gradient}}).
    `noise`: standard normals (Normal factors) or standard Gamma draws (Gamma factors), [K, ...].
    """
    leaves, draws, entropy = {}, {}, 0.0
    for name in noise:
        module = approx[name]
        cls = module.distribution_cls
        leaves[name] = {p: u.detach().cpu().double().requires_grad_()
                        for p, u in module.distribution_parameters.items()}
        args = {p: transform_to(cls.arg_constraints[p])(u) for p, u in leaves[name].items()}
        e = noise[name].detach().cpu().double()
        if cls is Normal:
            draws[name] = args["loc"] + e * args["scale"]
        else:
            draws[name] = _StandardGamma.apply(args["concentration"], e) / args["rate"]
        entropy = entropy + cls(**args).entropy().sum()
    total = log_joint(draws)
    assert total.shape == (K,)
    loss = -total.sum() / K - entropy
    loss.backward()
    return loss.detach(), {name: {p: u.grad for p, u in params.items()}
                           for name, params in leaves.items()}


def evaluate(model, approx, noise, monkeypatch, seed=11):
    """One ELBO evaluation and backward; returns (loss, loss module, the particle trace)."""
    traces = []
    original = particles.trace_particles

    def spy(*args, **kwargs):
        traces.append(original(*args, **kwargs))
        return traces[-1]
    monkeypatch.setattr(particles, "trace_particles", spy)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=seed)
    loss = loss_fn(model, approx(), _noise=noise)
    loss.backward()
    return loss, loss_fn, traces[-1]


def compare(loss, approx, want_loss, want_grads):
    close(loss, want_loss, VALUE_RTOL, VALUE_ATOL, "loss")
    for name, grads in want_grads.items():
        for pname, want in grads.items():
            got = approx[name].distribution_parameters[pname].grad
            close(got, want, GRAD_RTOL, GRAD_ATOL, f"grad {name}.{pname}")


def d64(x):
    return torch.as_tensor(x).detach().cpu().double()


def test_scale_priors_and_heavy_tails_against_float64(device, monkeypatch):
    """N = 1 (per-particle prior sites, Gamma guides) and N = 37 (the odd row tail)."""
    n = 37
    gen = torch.Generator().manual_seed(3)
    y = torch.randn(n, generator=gen) * 3
    w = torch.randn(n, generator=gen) * 2 + 0.5
    d = torch.randn(n, generator=gen).exp()

    def model():
        sigma = mi.sample("sigma", HalfCauchy(1.0))
        tau = mi.sample("tau", HalfNormal(2.0))
        lam = mi.sample("lam", Exponential(0.5))
        s = mi.sample("s", LogNormal(0.0, 1.0))
        mu = mi.sample("mu", Laplace(0.0, 2.0))
        mi.sample("y", Cauchy(mu, sigma), sample_shape=[n])
        mi.sample("w", StudentT(2.5, mu, tau + s), sample_shape=[n])
        mi.sample("d", TransformedDistribution(Normal(mu, lam), ExpTransform()), sample_shape=[n])

    approx, noise = guide_and_noise({
        "sigma": (Gamma, 3.0, 2.0), "tau": (Gamma, 2.0, 1.5), "lam": (Gamma, 4.0, 3.0),
        "s": (Gamma, 2.5, 2.5), "mu": (Normal, 0.3, 0.6)}, device, seed=5)
    cond = mi.condition(model, y=y.to(device), w=w.to(device), d=d.to(device))
    loss, _, trace = evaluate(cond, approx, noise, monkeypatch)
    assert trace.fallback == [], [name for name, _ in trace.fallback]
    assert {site.family for site in trace.sites} == {
        "half_cauchy", "half_normal", "exponential", "log_normal", "laplace", "cauchy",
        "student_t"}

    def log_joint(z):
        sigma, tau, lam, s, mu = (z[k].reshape(K, 1) for k in ("sigma", "tau", "lam", "s", "mu"))
        one = torch.ones((), dtype=torch.float64)
        prior = HalfCauchy(one).log_prob(sigma) + HalfNormal(2 * one).log_prob(tau) + \
            Exponential(0.5 * one).log_prob(lam) + LogNormal(0 * one, one).log_prob(s) + \
            Laplace(0 * one, 2 * one).log_prob(mu)
        return prior.sum(-1) + Cauchy(mu, sigma).log_prob(d64(y)).sum(-1) + \
            StudentT(2.5 * one, mu, tau + s).log_prob(d64(w)).sum(-1) + \
            TransformedDistribution(Normal(mu, lam), ExpTransform()).log_prob(d64(d)).sum(-1)
    compare(loss, approx, *reference_elbo(approx, noise, log_joint))


def robust_case(device, n=516):
    gen = torch.Generator().manual_seed(4)
    y = torch.randn(n, generator=gen) * 2
    mask = torch.rand(n, generator=gen) > 1 / 3
    z_loc = torch.linspace(-1, 1, n)
    z_scale = torch.linspace(0.5, 1.5, n)

    def model():
        sigma = mi.sample("sigma", Gamma(2.0, 2.0))
        z = mi.sample("z", Laplace(0.0, 1.0), sample_shape=[n])
        mi.sample("y", StudentT(4.0, z, sigma))

    approx = mi.nn.ParameterizedFactorizedDistribution(
        sigma=mi.nn.ParameterizedDistribution(Gamma, concentration=3.0, rate=2.0),
        z=mi.nn.ParameterizedDistribution(Normal, loc=z_loc, scale=z_scale)).to(device)
    cond = mi.condition(model, y=torch.masked.as_masked_tensor(y.to(device), mask.to(device)))
    return cond, approx, y, mask


def test_fused_draw_feeds_student_t_and_laplace_sites(device, monkeypatch):
    """N = 516: the lazy Normal draw z is made inside a site program that evaluates a masked
    StudentT(4., z, sigma) site and z's Laplace prior; z's noise is the generator's own
    (mi_philox_normal: stream 1, step 0), sigma's is injected."""
    n, seed = 516, 11
    cond, approx, y, mask = robust_case(device, n)
    g = torch._standard_gamma(torch.full((K,), 3.0), generator=torch.Generator().manual_seed(6))
    loss, loss_fn, trace = evaluate(cond, approx, {"sigma": g}, monkeypatch, seed=seed)
    assert trace.fallback == [], [name for name, _ in trace.fallback]
    assert [site.family for site in trace.sites] == ["gamma", "laplace", "student_t"]
    assert loss_fn.last_fusions["fused_draws"] == 1, loss_fn.last_fusions

    eps = torch.empty(K, n, device=device)
    nat.check(nat.lib().mi_philox_normal(K, n, seed, 0, 1, 0, eps.data_ptr(), None), "normals")
    torch.cuda.synchronize()

    def log_joint(s):
        sigma, z = s["sigma"].reshape(K, 1), s["z"]
        one = torch.ones((), dtype=torch.float64)
        lp = StudentT(4 * one, z, sigma).log_prob(d64(y))
        return Gamma(2 * one, 2 * one).log_prob(sigma).sum(-1) + \
            Laplace(0 * one, one).log_prob(z).sum(-1) + \
            torch.where(mask, lp, torch.zeros_like(lp)).sum(-1)
    compare(loss, approx, *reference_elbo(approx, {"sigma": g, "z": eps}, log_joint))


def test_count_likelihoods_against_float64(device, monkeypatch):
    """A batch(1000)-scaled NegativeBinomial(r, logits=a + b x) site observed at 37 rows and a
    Binomial(total_count=int tensor, probs=...) site."""
    n = 37
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(n, generator=gen)
    c = torch.poisson(torch.full((n,), 3.0), generator=gen)
    total = torch.randint(0, 12, (n,), generator=gen)
    m = torch.floor(total * torch.rand(n, generator=gen) + 0.5).clamp(max=total)
    xd, totald = x.to(device), total.to(device)

    def model():
        a = mi.sample("a", Normal(0.0, 1.0))
        b = mi.sample("b", Normal(0.0, 1.0))
        r = mi.sample("r", Gamma(2.0, 1.0))
        with mi.batch(1000):
            mi.sample("c", NegativeBinomial(r, logits=a + b * xd))
        mi.sample("m", Binomial(total_count=totald, probs=torch.sigmoid(a - b * xd)))

    approx, noise = guide_and_noise({"a": (Normal, 0.2, 0.5), "b": (Normal, -0.3, 0.4),
                                     "r": (Gamma, 4.0, 2.0)}, device, seed=9)
    cond = mi.condition(model, c=c.to(device), m=m.to(device))
    loss, _, trace = evaluate(cond, approx, noise, monkeypatch)
    assert trace.fallback == [], [name for name, _ in trace.fallback]
    families = {site.name: site.family for site in trace.sites}
    assert families["c"] == "negative_binomial" and families["m"] == "binomial"
    assert next(site for site in trace.sites if site.name == "c").scale == 1000 / n

    def log_joint(z):
        a, b, r = (z[k].reshape(K, 1) for k in ("a", "b", "r"))
        one = torch.ones((), dtype=torch.float64)
        prior = Normal(0 * one, one).log_prob(a) + Normal(0 * one, one).log_prob(b) + \
            Gamma(2 * one, one).log_prob(r)
        return prior.sum(-1) + \
            (1000 / n) * NegativeBinomial(r, logits=a + b * d64(x)).log_prob(d64(c)).sum(-1) + \
            Binomial(total_count=total, probs=torch.sigmoid(a - b * d64(x))) \
            .log_prob(d64(m)).sum(-1)
    compare(loss, approx, *reference_elbo(approx, noise, log_joint))


def test_validation_errors_carry_the_site_name(device):
    n = 37

    def model():
        z = mi.sample("z", Laplace(0.0, scale), sample_shape=[n])
        mi.sample("c", NegativeBinomial(2.5, logits=z))

    approx = mi.nn.ParameterizedFactorizedDistribution(
        z=mi.nn.ParameterizedDistribution(Normal, loc=torch.zeros(n),
                                          scale=torch.ones(n))).to(device)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=1, validate=True)
    counts = torch.full((n,), 2.0, device=device)
    scale = 1.0
    loss_fn(mi.condition(model, c=counts), approx())
    bad = counts.clone()
    bad[5] = 1.5
    with pytest.raises(ValueError, match="Parameter 'c' is not in the support of NegativeBinomial"):
        loss_fn(mi.condition(model, c=bad), approx())
    scale = -1.0
    with pytest.raises(ValueError, match="distribution Laplace for site 'z'"):
        loss_fn(mi.condition(model, c=counts), approx())


def test_captured_step_of_the_fused_draw_model(device):
    """A StepGraph step (loss and backward) of the N = 516 model: replays run the site program
    with the StudentT and Laplace sites, draw anew each time, and reproduce the eager step at the
    same generator counter bit for bit."""
    def setup():
        cond, approx, _, _ = robust_case(device)
        loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=7)

        def step():
            approx.zero_grad(set_to_none=True)
            loss = loss_fn(cond, approx())
            loss.backward()
            return loss
        return step, loss_fn, approx

    eager_step, eager_fn, eager_approx = setup()
    eager = [float(eager_step()) for _ in range(3)]
    assert eager_fn.last_fusions["fused_draws"] == 1
    eager_grad = eager_approx["z"].distribution_parameters["loc"].grad.clone()
    body, graph_fn, graph_approx = setup()
    captured = StepGraph(body, warmup=2)   # warm-up: counters 0 and 1; the replays: 2 and 3
    first = float(captured())
    first_grad = graph_approx["z"].distribution_parameters["loc"].grad.clone()
    second = float(captured())
    captured.check()
    assert graph_fn.last_fusions["fused_draws"] == 1
    assert first == eager[2]
    assert torch.equal(first_grad, eager_grad)
    assert second != first and np.isfinite(second)
