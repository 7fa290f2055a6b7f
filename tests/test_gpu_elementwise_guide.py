"""
The native Exponential, Laplace, Cauchy, HalfCauchy, HalfNormal and LogNormal guide factors on the
MI355X: mi_elementwise_rsample against the float64 restatement from the oracle's Philox words
(tests/elementwise_reference.py, itself checked against torch float64 on the host), its backward
against float64 sums of the float32 noise, mi_elementwise_entropy against torch float64, and the
factors through EvidenceLowerBoundLoss (parity with float64 torch under injected noise, seed
governance, particle shards, a captured training step).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch.distributions import (Exponential, Gamma, Laplace, LogNormal, Normal, Poisson,
                                 TransformedDistribution)
from torch.distributions.transforms import ExpTransform

import mininf_amd as mi
from mininf_amd import _native as nat, guide
from mininf_amd.graph import StepGraph
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution
from tests import elementwise_reference as ref
from tests import predictive_reference as pr

pytestmark = pytest.mark.gpu

SEED, STEP, STREAM, OFFSET = ref.SEED, ref.STEP, ref.STREAM, ref.OFFSET
SUM_ROUNDING = 4 * 2.0 ** -24   # the particle sums' own rounding


def host64(t):
    return t.cpu().numpy().astype(np.float64)


def on_device(device, params):
    return [torch.as_tensor(p, dtype=torch.float32, device=device).contiguous() for p in params]


def strides(params, N):
    return [1 if len(p) == N and N > 1 else 0 for p in params]


def rsample(device, family, params, K, N, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET,
            noise=None, step_device=None, out=None):
    held = on_device(device, params)
    s = strides(params, N)
    z = torch.full((K, N), float("nan"), device=device) if out is None else out
    b = held[1] if len(held) > 1 else None
    nat.check(nat.lib().mi_elementwise_rsample(
        ref.CODE[family], held[0].data_ptr(), s[0], nat.ptr(b), s[1] if b is not None else 0, K, N,
        seed, step, nat.ptr(step_device), stream_id, offset, nat.ptr(noise), z.data_ptr(), None),
        "mi_elementwise_rsample")
    return z


def workspace_bytes(K, N):
    size = ctypes.c_size_t()
    nat.check(nat.lib().mi_elementwise_rsample_backward_workspace_bytes(K, N, ctypes.byref(size)),
              "workspace")
    return size.value


def rsample_backward(device, family, params, dz, K, N, seed=SEED, step=STEP, stream_id=STREAM,
                     offset=OFFSET, noise=None, step_device=None, want=(True, True)):
    held = on_device(device, params)
    s = strides(params, N)
    b = held[1] if len(held) > 1 else None
    size = workspace_bytes(K, N)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=device)
    da = torch.full((N,), float("nan"), device=device) if want[0] else None
    db = torch.full((N,), float("nan"), device=device) if want[1] and b is not None else None
    nat.check(nat.lib().mi_elementwise_rsample_backward(
        ref.CODE[family], dz.data_ptr(), dz.stride(0), dz.stride(1), held[0].data_ptr(), s[0],
        nat.ptr(b), s[1] if b is not None else 0, K, N, seed, step, nat.ptr(step_device),
        stream_id, offset, nat.ptr(noise), ws.data_ptr(), size, nat.ptr(da), nat.ptr(db), None),
        "mi_elementwise_rsample_backward")
    return da, db


def device_noise(device, family, K, N, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET):
    """The float32 base noise the kernels read: the exact u01 of the oracle's words, or the
    device's own normals (mi_philox_normal)."""
    if family not in ref.NORMAL_BASED:
        u = ref.uniforms(K, N, seed=seed, step=step, stream_id=stream_id, offset=offset)
        return torch.as_tensor(u, device=device).contiguous()
    eps = torch.empty((K, N), device=device)
    nat.check(nat.lib().mi_philox_normal(K, N, seed, step, stream_id, offset, eps.data_ptr(), None),
              "mi_philox_normal")
    return eps


def check_draws(family, params, z, v64, N):
    """Finite, inside the support, and within the family's bound of the restatement."""
    got = host64(z)
    assert np.isfinite(got).all()
    if family in ref.POSITIVE:
        assert (got > 0).all()
    want = ref.draw(family, params, v64)
    keep = pr.tangent_compared(v64) if "cauchy" in family else np.ones(v64.shape, bool)
    assert (~keep).sum() <= ref.LEFT_OUT_CAP * keep.size   # a condition, not a measurement
    full = [np.broadcast_to(p, want.shape) for p in params]
    error = pr.relative_error(family, [p[keep] for p in full], got[keep], want[keep])
    largest = error.max() if error.size else 0.0
    assert largest <= ref.DRAW_RTOL[family], (largest, ref.DRAW_RTOL[family])
    return largest


# ---- 1. the draw against the restatement -------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N", ref.NS)
@pytest.mark.parametrize("K", ref.KS)
def test_draw_matches_restatement(device, family, N, K):
    """step != 0 and particle_offset != 0 throughout; dense and stride-0 parameters; an unaligned
    z; rows at an offset; the device's own noise injected."""
    v64 = ref.noise(family, K, N)
    dense = ref.parameters(family, N, "dense")
    z = rsample(device, family, dense, K, N)
    worst = check_draws(family, dense, z, v64, N)
    scalar = ref.parameters(family, N, "scalar")
    worst = max(worst, check_draws(family, scalar, rsample(device, family, scalar, K, N), v64, N))
    print(f"{family} N={N} K={K}: largest relative error {worst:.3g} "
          f"({worst / ref.DRAW_RTOL[family]:.3g} of the bound)")
    # a view offset by one float: no 16-byte store may be issued, nothing beside z is written
    buffer = torch.full((K * N + 2,), float("nan"), device=device)
    shifted = rsample(device, family, dense, K, N, out=buffer[1:K * N + 1].view(K, N))
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(shifted, z)
    assert torch.isnan(buffer[0]) and torch.isnan(buffer[-1])
    # row k at offset o is row k + o at offset 0
    whole = rsample(device, family, dense, K + OFFSET, N, offset=0)
    assert torch.equal(whole[OFFSET:], z)
    # the device's own noise, injected, reproduces the draw (neither seed nor step is read)
    noise = device_noise(device, family, K, N)
    again = rsample(device, family, dense, K, N, noise=noise, seed=SEED + 1, step=STEP + 1)
    assert torch.equal(again, z)
    assert torch.equal(rsample(device, family, dense, K, N), z)


@pytest.mark.parametrize("family", ("half_normal", "log_normal"))
@pytest.mark.parametrize("N", (5, 257))
def test_normal_based_draws_use_the_normal_factors_eps(device, family, N):
    """scale |eps| and exp(loc + scale eps) of mi_philox_normal's eps, at 2e-7."""
    K = 33
    params = ref.parameters(family, N)
    eps = host64(device_noise(device, family, K, N))
    got = host64(rsample(device, family, params, K, N))
    want = ref.draw(family, params, eps)
    assert (np.abs(got - want) <= 2e-7 * np.abs(want)).all(), (np.abs(got / want - 1)).max()


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_grid_corners_stay_inside_the_support(device, family):
    """Injected u at u01(0) and u01(0xFFFFFFFF) = 1.0f (eps of +-5.9 and 0.1 for the normal-based
    families): finite draws, positive ones for the four positive families."""
    corners = pr.u01(np.array([0, 0xFFFFFFFF], np.uint32))
    if family in ref.NORMAL_BASED:
        corners = np.array([-5.9, 5.9, 0.1], np.float32)
    K, N = len(corners), 5
    v = np.repeat(corners[:, None], N, axis=1)
    params = ref.parameters(family, N)
    noise = torch.as_tensor(v, dtype=torch.float32, device=device).contiguous()
    z = rsample(device, family, params, K, N, noise=noise)
    if "cauchy" not in family:   # (the tangents' corners lie in the band left out)
        check_draws(family, params, z, ref.clamp(family, v), N)
    got = host64(z)
    assert np.isfinite(got).all()
    if family in ref.POSITIVE:
        assert (got > 0).all()


def test_device_step_counter(device):
    """The step read from the device word (graph replays) is the same stream as the argument."""
    K, N = 33, 257
    counter = torch.tensor([7], dtype=torch.int64, device=device)
    for family in ("exponential", "log_normal"):
        params = ref.parameters(family, N)
        by_word = rsample(device, family, params, K, N, step=0, step_device=counter)
        assert torch.equal(by_word, rsample(device, family, params, K, N, step=7))
        assert not torch.equal(by_word, rsample(device, family, params, K, N, step=6))
        dz = torch.randn(K, N, generator=torch.Generator().manual_seed(1)).to(device)
        a = rsample_backward(device, family, params, dz, K, N, step=0, step_device=counter)
        b = rsample_backward(device, family, params, dz, K, N, step=7)
        assert all(x is None or torch.equal(x, y) for x, y in zip(a, b))


# ---- 2. the backward against float64 -----------------------------------------------------------
# (1025, 1): more than one particle slice of a one-element factor
BACKWARD_SHAPES = [(K, N) for N in ref.NS for K in ref.KS] + [(1025, 1)]


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N", BACKWARD_SHAPES)
def test_backward_matches_float64(device, family, K, N):
    """da = sum_k dz dz/da within (4 2^-24 + the family's draw bound) sum_k |dz dz/da|, the float64
    reference from the float32 noise; dz contiguous, stored transposed and as a padded view."""
    rng = np.random.default_rng(7 + 1000 * N + K)
    params = ref.parameters(family, N)
    noise = device_noise(device, family, K, N)
    fa, fb = ref.factors(family, params, host64(noise))
    dz64 = rng.standard_normal((K, N)).astype(np.float32).astype(np.float64)
    rel = SUM_ROUNDING + ref.DRAW_RTOL[family]
    wants = [((dz64 * f).sum(0), rel * np.abs(dz64 * f).sum(0)) for f in (fa, fb) if f is not None]
    contiguous = torch.as_tensor(dz64, dtype=torch.float32, device=device)
    transposed = contiguous.t().contiguous().t()          # strides (1, K)
    padded = torch.zeros(K, N + 3, device=device)[:, 1:N + 1]   # row stride N + 3, offset view
    padded.copy_(contiguous)
    first, used = None, 0.0
    for dz in (contiguous, transposed, padded):
        got = [g for g in rsample_backward(device, family, params, dz, K, N) if g is not None]
        assert len(got) == len(wants)
        # the kernels read the same values in the same order whatever the strides
        first = first or got
        assert all(torch.equal(g, f) for g, f in zip(got, first))
        for g, (want, bound) in zip(got, wants):
            err = np.abs(host64(g) - want)   # NaN (an unwritten element) fails the comparison
            used = max(used, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (err / bound).max()
    print(f"{family} K={K} N={N} slices={'>1' if workspace_bytes(K, N) else '1'}: "
          f"largest fraction of the bound used {used:.3g}")
    # injected noise reads the same values; one output alone is the same output
    injected = rsample_backward(device, family, params, contiguous, K, N, noise=noise,
                                seed=SEED + 1, step=STEP + 1)
    assert all(torch.equal(g, f) for g, f in zip([g for g in injected if g is not None], first))
    if family in ref.TWO_PARAMETERS:
        only_b = rsample_backward(device, family, params, contiguous, K, N, want=(False, True))
        assert only_b[0] is None and torch.equal(only_b[1], first[1])


def test_backward_shapes_cover_one_and_many_slices():
    sizes = {(K, N): workspace_bytes(K, N) for K, N in BACKWARD_SHAPES}
    assert sizes[(1, 1)] == 0 and sizes[(64, 1)] == 0 and sizes[(1, 1030)] == 0
    assert sizes[(1025, 1)] > 0 and sizes[(64, 257)] > 0 and sizes[(33, 1030)] > 0


# ---- 3. the entropy against torch float64 ------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N", ref.ENTROPY_NS)
def test_entropy_matches_torch_float64(device, family, N):
    params = ref.entropy_parameters(family, N)
    leaves = [torch.as_tensor(p, dtype=torch.float64).clone().requires_grad_() for p in params]
    want = ref.torch_distribution(family, leaves).entropy().sum()
    want.backward()
    held = on_device(device, params)
    b = held[1] if len(held) > 1 else None
    H = torch.full((), float("nan"), device=device)
    da = torch.full((N,), float("nan"), device=device)
    db = torch.full((N,), float("nan"), device=device) if b is not None else None
    nat.check(nat.lib().mi_elementwise_entropy(
        ref.CODE[family], held[0].data_ptr(), 1, nat.ptr(b), 1, N, H.data_ptr(), da.data_ptr(),
        nat.ptr(db), None), "mi_elementwise_entropy")
    assert abs(float(H) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    for got, leaf in zip((da, db), leaves):
        grad = leaf.grad.numpy() if leaf.grad is not None else np.zeros(N)
        assert (np.abs(host64(got) - grad) <= 1e-5 * np.abs(grad)).all()
    # the value alone; stride-0 parameters
    alone = torch.full((), float("nan"), device=device)
    nat.check(nat.lib().mi_elementwise_entropy(
        ref.CODE[family], held[0].data_ptr(), 1, nat.ptr(b), 1, N, alone.data_ptr(), None, None,
        None), "mi_elementwise_entropy")
    assert torch.equal(alone, H)
    scalar = torch.full((), float("nan"), device=device)
    nat.check(nat.lib().mi_elementwise_entropy(
        ref.CODE[family], held[0].data_ptr(), 0, nat.ptr(b), 0, N, scalar.data_ptr(), None, None,
        None), "mi_elementwise_entropy")
    one = ref.torch_distribution(family, [t[:1].detach() for t in leaves]).entropy().sum()
    assert abs(float(scalar) - N * float(one)) <= 1e-5 * abs(N * float(one))


# ---- 4. through the loss -----------------------------------------------------------------------
N_OBS, N_ROWS, P = 37, 96, 5


@functools.lru_cache(maxsize=None)
def data():
    gen = torch.Generator().manual_seed(0)
    y = 1.3 * torch.randn(N_OBS, generator=gen)
    X = torch.randn(N_ROWS, P, generator=gen) / P ** 0.5
    t = X @ torch.randn(P, generator=gen) + torch.randn(N_ROWS, generator=gen)
    counts = torch.poisson(torch.full((N_OBS,), 3.0), generator=gen)
    return y, X, t, counts


def case(name, device):
    """(conditioned model, site name, ParameterizedDistribution, parameter names,
    float64 log joint of [K, *shape] draws, float64 factor of leaves)."""
    y, X, t, counts = data()
    one = torch.ones((), dtype=torch.float64)
    if name == "a":
        def model():
            sigma = mi.sample("sigma", Gamma(2.0, 2.0))
            mi.sample("y", Normal(0.0, sigma), sample_shape=[N_OBS])

        module = ParameterizedDistribution(LogNormal, loc=torch.tensor(0.2),
                                           scale=torch.tensor(0.3))

        def log_joint(z):
            z = z.reshape(-1, 1)
            return Gamma(2 * one, 2 * one).log_prob(z).sum(-1) + \
                Normal(0 * one, z).log_prob(y.double()).sum(-1)

        def factor(leaves):
            return LogNormal(leaves["loc"], leaves["scale"].exp())
        return mi.condition(model, y=y.to(device)), "sigma", module, ("loc", "scale"), \
            log_joint, factor
    if name == "b":
        Xd = X.to(device)

        def model():
            theta = mi.sample("theta", Normal(0.0, 1.0), (P,))
            mi.sample("y", Normal(Xd @ theta, 1.0))

        module = ParameterizedDistribution(Laplace, loc=torch.linspace(-0.3, 0.3, P),
                                           scale=torch.linspace(0.2, 0.6, P))

        def log_joint(z):
            return Normal(0 * one, one).log_prob(z).sum(-1) + \
                Normal(z @ X.double().T, one).log_prob(t.double()).sum(-1)

        def factor(leaves):
            return Laplace(leaves["loc"], leaves["scale"].exp())
        return mi.condition(model, y=t.to(device)), "theta", module, ("loc", "scale"), \
            log_joint, factor

    def model():
        lam = mi.sample("lam", Gamma(2.0, 1.0))
        mi.sample("c", Poisson(lam), sample_shape=[N_OBS])

    module = ParameterizedDistribution(Exponential, rate=torch.tensor(0.4))

    def log_joint(z):
        z = z.reshape(-1, 1)
        return Gamma(2 * one, one).log_prob(z).sum(-1) + \
            Poisson(z).log_prob(counts.double()).sum(-1)

    def factor(leaves):
        return Exponential(leaves["rate"].exp())
    return mi.condition(model, c=counts.to(device)), "lam", module, ("rate",), log_joint, factor


FAMILY_OF = {"a": "log_normal", "b": "laplace", "c": "exponential"}


def base_noise(name, K):
    shape = (K, P) if name == "b" else (K,)
    gen = torch.Generator().manual_seed(100 + K)
    if FAMILY_OF[name] in ref.NORMAL_BASED:
        return torch.randn(shape, generator=gen)
    # uniforms on the generator's own 24-bit grid
    bits = torch.randint(0, 1 << 24, shape, generator=gen)
    return ((bits.double() + 0.5) * 2.0 ** -24).float().clamp(max=1.0 - 2.0 ** -24)


def evaluate(name, device, K, seed, noise=None, offset=None):
    """Loss, unconstrained-parameter gradients and fusions of one evaluation with a fresh loss and
    guide; with ``offset``, the draws of K particles at that particle offset instead."""
    model, site, module, names, _, _ = case(name, device)
    module = module.to(device)
    init = {n: module.distribution_parameters[n].detach().cpu().double().clone() for n in names}
    if offset is not None:
        return guide.draw_all({site: module()}, K, seed, 0, offset)[site].detach().clone()
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=seed)
    extra = {} if noise is None else {"_noise": {site: noise}}
    loss = loss_fn(model, {site: module()}, **extra)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: module.distribution_parameters[n].grad.detach().clone() for n in names}
    return loss.detach().clone(), grads, dict(loss_fn.last_fusions), init


def reference(name, init, noise, dtype=torch.float64):
    """torch on the host: the factor built from the same unconstrained parameters, its draws from
    the same base noise by the kernels' transform, its own entropy."""
    _, _, _, names, log_joint, factor = case(name, torch.device("cpu"))
    leaves = {n: init[n].to(dtype).clone().requires_grad_() for n in names}
    f = factor(leaves)
    v = noise.to(dtype)
    if name == "a":
        z = (f.loc + f.scale * v).exp()
    elif name == "b":
        d = v - 0.5
        z = f.loc - f.scale * d.sign() * torch.log1p(-2 * d.abs())
    else:
        z = -v.log() / f.rate
    loss = -log_joint(z.double()).mean().to(dtype) - f.entropy().sum()
    loss.backward()
    return loss.detach(), {n: leaves[n].grad for n in names}


@pytest.mark.parametrize("name", ("a", "b", "c"))
@pytest.mark.parametrize("K", (8, 40))
def test_loss_matches_float64_torch_under_injected_noise(device, name, K):
    """The project's table tolerances, unchanged: loss within 1e-5 relative, every guide gradient
    within 2e-5 of its vector's max-norm."""
    noise = base_noise(name, K)
    loss, grads, fusions, init = evaluate(name, device, K, seed=21, noise=noise)
    assert fusions["elementwise_draws"] == 1
    want, want_grads = reference(name, init, noise)
    rel = abs(float(loss) - float(want)) / abs(float(want))
    print(f"model ({name}) K={K}: loss {float(loss):.8g} reference {float(want):.8g}: "
          f"{rel / 1e-5:.3g} of the bound")
    failures = [] if rel <= 1e-5 else [("loss", rel)]
    for n, ref_grad in want_grads.items():
        scale = float(ref_grad.abs().max())
        err = float((grads[n].cpu().double().reshape(ref_grad.shape) - ref_grad).abs().max())
        print(f"  d{n}: {err / scale / 2e-5:.3g} of the bound")
        if not err / scale <= 2e-5:
            failures.append((n, err / scale))
    assert not failures, failures


def test_loss_is_governed_by_its_seed(device):
    """No injected noise: torch's generator plays no part, and two half-K evaluations at particle
    offsets 0 and K / 2 draw the rows of the full run."""
    K = 40
    torch.manual_seed(1)
    loss_a, grads_a, fusions, _ = evaluate("a", device, K, seed=7)
    assert fusions["elementwise_draws"] == 1
    torch.manual_seed(2)
    loss_b, grads_b, _, _ = evaluate("a", device, K, seed=7)
    assert torch.isfinite(loss_a)
    assert torch.equal(loss_a, loss_b)
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n
    loss_c, _, _, _ = evaluate("a", device, K, seed=8)
    assert not torch.equal(loss_a, loss_c)
    whole = evaluate("a", device, K, seed=7, offset=0)
    torch.manual_seed(3)
    first = evaluate("a", device, K // 2, seed=7, offset=0)
    second = evaluate("a", device, K // 2, seed=7, offset=K // 2)
    assert whole.shape == (K,) and (whole > 0).all()
    assert torch.equal(whole[:K // 2], first) and torch.equal(whole[K // 2:], second)


def test_declined_factors_keep_torchs_path(device):
    class MyLogNormal(LogNormal):
        pass

    loc, scale = torch.tensor(0.2, device=device), torch.tensor(0.3, device=device)
    assert guide.native_elementwise(LogNormal(loc, scale))
    assert guide.native_elementwise(Exponential(scale.expand(3)))
    declined = (MyLogNormal(loc, scale), LogNormal(loc.double(), scale.double()),
                LogNormal(loc.cpu(), scale.cpu()),
                TransformedDistribution(Normal(loc, scale), ExpTransform()))
    for factor in declined:
        assert not guide.native_elementwise(factor)
    model = case("a", device)[0]
    loss_fn = EvidenceLowerBoundLoss(num_particles=8, seed=1)
    module = ParameterizedDistribution(MyLogNormal, loc=torch.tensor(0.2),
                                       scale=torch.tensor(0.3)).to(device)
    loss = loss_fn(model, {"sigma": module()})
    loss.backward()
    assert loss_fn.last_fusions["elementwise_draws"] == 0
    assert torch.isfinite(loss)
    for p in module.distribution_parameters.values():
        assert p.grad is not None and torch.isfinite(p.grad).all()


# ---- 5. captured step --------------------------------------------------------------------------
def training_setup(device):
    model, site, module, _, _, _ = case("a", device)
    module = module.to(device)
    optimizer = mi.optim.Adam(module.parameters(), lr=0.01)
    loss_fn = EvidenceLowerBoundLoss(num_particles=40, seed=17)

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(model, {site: module()})
        loss.backward()
        optimizer.step()
        return loss

    return step, module, loss_fn


def test_captured_step_draws_anew_on_every_replay(device):
    eager_step, eager_module, eager_loss_fn = training_setup(device)
    eager = [float(eager_step()) for _ in range(3)]
    assert eager_loss_fn.last_fusions["elementwise_draws"] == 1
    assert len(set(eager)) == 3
    # one eager warm-up step, then the capture of step 1 (not executed) and two replays
    graph_body, graph_module, _ = training_setup(device)
    captured = StepGraph(graph_body, warmup=1)
    replayed = [float(captured()) for _ in range(2)]
    captured.check()
    torch.testing.assert_close(torch.tensor(replayed), torch.tensor(eager[1:]), rtol=1e-6, atol=0)
    for a, b in zip(eager_module.parameters(), graph_module.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
