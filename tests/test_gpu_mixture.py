"""
The Normal-mixture site (``mi_mixture_normal_forward``), its place in the ELBO step and its
predictive draw (``mi_predictive_mixture_normal``) on the GPU.

Kernel: point by point against the float64 closed form (tests/mixture_reference.py) on the same
float32 inputs. The error of ``total[k]`` is taken relative to scale * sum_i mask_i (max_c |t_ic| +
1), of each gradient entry relative to |g0 * scale| times the sum of the absolute terms of its
formula, of a drawn value relative to |loc_c| + |scale_c eps|. Each bound is 4 x the larger of the
kernel's largest measured fraction on the MI355X and the fraction torch float32 reaches on the host
on the same cases (MEASURED below; DESIGN.md 0k records both).

dloc and dscale are single products with r_c, so an r_c below float32's range (float64 still holds
it) makes a float32 entry's error all of its size: that fraction is 1 for the kernel and for torch
float32 alike (beside float32's denormals it exceeds 1) and the bound over all entries checks
little. The entries with r_c >= 2^-64 are therefore
bounded a second time on their own ("clear").

Through the loss the bounds are the project's table: 1e-5 relative for the loss, 2e-5 of each
gradient vector's max-norm, against float64 torch on the host.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch.distributions import (Categorical, Dirichlet, LogNormal, MixtureSameFamily, Normal,
                                 transform_to)

import mininf_amd as mi
from mininf_amd import _native as nat, engine, particles, predictive
from mininf_amd.graph import StepGraph
from mininf_amd.nn import (EvidenceLowerBoundLoss, ParameterizedDistribution,
                           ParameterizedFactorizedDistribution)
from tests import dirichlet_reference as dref
from tests import mixture_reference as mref

pytestmark = pytest.mark.gpu

# name: (kernel's largest fraction on the MI355X, torch float32's on the host), over every case of
# test_kernel_against_closed_form and test_kernel_special_rows
MEASURED = {
    "total": (1.45e-7, 9.76e-8),
    "dlogits": (7.6e-7, 1.6e-6),
    "dloc": (1.29, 2.24),
    "dscale": (1.3, 1.01),
    "dvalue": (4.33e-7, 6.25e-7),
    "dloc_clear": (1.16e-5, 1.29e-5),
    "dscale_clear": (1.13e-5, 1.24e-5),
    "draw": (1.81e-7, 1.27e-7),   # (the second figure: the float32 restatement of the draw)
}
BOUND = {name: 4.0 * max(pair) for name, pair in MEASURED.items()}
GUARD = 64
SENTINEL = -12345.0


def on_device(a, device, full=None):
    """The array on the device, expanded (stride 0) to ``full`` when given."""
    t = torch.as_tensor(np.ascontiguousarray(a), device=device)
    return t if full is None else t.expand(full)


def guarded(shape, device, dtype=torch.float32):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=device)
    return flat, flat[:n].view(shape)


def launch(device, logits, loc, scale, x, mask=None, batch_scale=1.0, g0=1.0,
           need=(True, True, True, True)):
    """mi_mixture_normal_forward on [K, N, C] views of the arrays (stride 0 along a broadcast
    axis): a dict with total, the four gradients (None when not asked for) and flags; checks the
    guard words after every output and after the workspace."""
    K, N, C = np.broadcast_shapes(logits.shape, loc.shape, scale.shape, x.shape + (1,))
    params = [on_device(a, device, (K, N, C)) for a in (logits, loc, scale)]
    xv = on_device(x, device, (K, N))
    mv = None if mask is None else on_device(np.asarray(mask, np.uint8), device)
    lib = nat.lib()
    size = ctypes.c_size_t()
    assert lib.mi_mixture_normal_workspace_bytes(K, N, C, ctypes.byref(size)) == 0
    assert size.value % 8 == 0
    ws_flat, ws = guarded((size.value // 8,), device, torch.float64)
    outs = [guarded((K, N, C), device) if wanted else (None, None) for wanted in need[:3]]
    outs.append(guarded((K, N), device) if need[3] else (None, None))
    total_flat, total = guarded((K,), device)
    flags_flat, flags = guarded((1,), device, torch.int32)
    strided = [v for t in params for v in (t.data_ptr(), *t.stride())]
    code = lib.mi_mixture_normal_forward(
        *strided, K, N, C, xv.data_ptr(), xv.stride(0), xv.stride(1), nat.ptr(mv),
        0 if mv is None else mv.stride(0), batch_scale, g0, *[nat.ptr(o[1]) for o in outs],
        ws.data_ptr(), size.value, total.data_ptr(), flags.data_ptr(), nat.stream_handle(device))
    assert code == 0, code
    torch.cuda.synchronize()
    for flat in [ws_flat, total_flat] + [o[0] for o in outs if o[0] is not None]:
        assert bool((flat[-GUARD:] == SENTINEL).all())
    assert bool((flags_flat[-GUARD:] == int(SENTINEL)).all())
    out = {name: None if o[1] is None else o[1].cpu().numpy()
           for name, o in zip(mref.GRADS, outs)}
    out.update(total=total.cpu().numpy(), flags=int(flags.cpu()[0]))
    return out


WORST = {}


def check(what, got, want, inputs=None, **kwargs):
    """Print and bound the fractions of one case (and torch float32's, where inputs are given)."""
    mine = mref.fractions(got, want)
    theirs = mref.fractions(mref.torch_float32(*inputs, **kwargs), want) if inputs else {}
    for name, value in mine.items():
        pair = WORST.setdefault(name, [0.0, 0.0])
        pair[0], pair[1] = max(pair[0], value), max(pair[1], theirs.get(name, 0.0))
    print(what, " ".join(f"{n}={v:.3g}/{theirs.get(n, float('nan')):.3g}" for n, v in mine.items()))
    print("  largest so far (kernel, torch float32):",
          {n: (f"{a:.3g}", f"{b:.3g}") for n, (a, b) in WORST.items()})
    for name, value in mine.items():
        assert value <= BOUND[name], (what, name, value, BOUND[name])


@pytest.mark.parametrize("layout", mref.LAYOUTS)
@pytest.mark.parametrize("C", mref.KERNEL_C)
def test_kernel_against_closed_form(device, C, layout):
    for N, K in itertools.product(mref.KERNEL_N, mref.KERNEL_K):
        inputs = mref.kernel_case(C, N, K, layout)
        got = launch(device, *inputs)
        assert got["flags"] == 0
        check(f"C={C} N={N} K={K} {layout}:", got, mref.closed_form(*inputs), inputs)


@pytest.mark.parametrize("C", [3, 65])
def test_kernel_mask_and_scale(device, C):
    K, N = 7, 5
    inputs = mref.kernel_case(C, N, K)
    mask = np.array([1, 0, 1, 1, 0], bool)
    kwargs = dict(mask=mask, batch_scale=2.5, g0=-1.0 / K)
    got = launch(device, *inputs, **kwargs)
    check(f"masked C={C}:", got, mref.closed_form(*inputs, **kwargs), inputs, **kwargs)
    for name in mref.GRADS:
        assert np.all(got[name][:, ~mask] == 0), name


def test_kernel_special_rows(device):
    # a component of logit -inf: r_c = 0, exact zero gradients, nothing NaN
    logits, loc, scale, x = mref.kernel_case(5, 3, 2)
    logits = logits.copy()
    logits[:, :, 2] = -np.inf
    got = launch(device, logits, loc, scale, x)
    assert got["flags"] == 0
    for name in mref.GRADS[:3]:
        assert np.all(got[name][:, :, 2] == 0), name
    assert all(np.isfinite(got[name]).all() for name in ("total",) + mref.GRADS)
    check("-inf logit:", got, mref.closed_form(logits, loc, scale, x))
    # a row 40 standard deviations from every component: finite, and sum_c r_c = 1
    inputs = mref.far_case()
    got = launch(device, *inputs)
    want = mref.closed_form(*inputs)
    assert got["flags"] == 0 and np.isfinite(got["total"]).all()
    check("far row:", got, want, inputs)
    # r_c - exp(m_c) summed over c is sum_c r_c - 1
    np.testing.assert_allclose(got["dlogits"].astype(np.float64).sum(-1), 0.0, atol=4 * 2.0 ** -23)


def test_null_gradients_and_determinism(device):
    inputs = mref.kernel_case(33, 5, 7)
    full = launch(device, *inputs)
    again = launch(device, *inputs)
    for name in ("total",) + mref.GRADS:
        assert np.array_equal(full[name], again[name]), name
    for j, name in enumerate(mref.GRADS):
        need = tuple(i != j for i in range(4))
        part = launch(device, *inputs, need=need)
        assert part[name] is None and np.array_equal(part["total"], full["total"])
        for other in mref.GRADS:
            if other != name:
                assert np.array_equal(part[other], full[other]), (name, other)
    none = launch(device, *inputs, need=(False,) * 4)
    assert np.array_equal(none["total"], full["total"])


def test_validation_flags(device):
    logits, loc, scale, x = (a.copy() for a in mref.kernel_case(3, 5, 2))
    mask = np.array([1, 1, 0, 1, 1], bool)
    bad_scale = scale.copy()
    bad_scale[1, 2, 1] = 0.0
    assert launch(device, logits, loc, bad_scale, x)["flags"] == nat.FLAG_PARAM
    assert launch(device, logits, loc, bad_scale, x, mask=mask)["flags"] == 0
    empty = logits.copy()
    empty[0, 2, :] = -np.inf
    assert launch(device, empty, loc, scale, x)["flags"] == nat.FLAG_PARAM
    assert launch(device, empty, loc, scale, x, mask=mask)["flags"] == 0
    nan_logit = logits.copy()
    nan_logit[0, 2, 0] = np.nan
    assert launch(device, nan_logit, loc, scale, x)["flags"] == nat.FLAG_PARAM
    nan_x = x.copy()
    nan_x[1, 2] = np.nan
    assert launch(device, logits, loc, scale, nan_x)["flags"] == nat.FLAG_SUPPORT
    assert launch(device, logits, loc, scale, nan_x, mask=mask)["flags"] == 0


def test_arguments_are_checked_before_any_launch(device):
    lib = nat.lib()
    size = ctypes.c_size_t()
    C = nat.MIXTURE_MAX_C + 1
    assert lib.mi_mixture_normal_workspace_bytes(1, 1, C, ctypes.byref(size)) == nat.MI_EUNSUPPORTED
    assert lib.mi_mixture_normal_workspace_bytes(0, 1, 3, ctypes.byref(size)) == nat.MI_EINVAL
    buf = torch.full((2 * C + GUARD,), SENTINEL, device=device)
    p = buf.data_ptr()
    stream = nat.stream_handle(device)

    def call(logits, K, N, C):
        return lib.mi_mixture_normal_forward(logits, 0, 0, 1, p, 0, 0, 1, p, 0, 0, 1, K, N, C, p,
                                             0, 0, None, 0, 1.0, 1.0, None, None, None, None, p,
                                             8, p, p, stream)
    assert call(p, 1, 1, C) == nat.MI_EUNSUPPORTED
    assert call(None, 1, 1, 3) == nat.MI_EINVAL
    assert call(p, 1, 0, 3) == nat.MI_EINVAL and call(p, 1, 1, 0) == nat.MI_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())   # nothing ran: total, flags and workspace untouched


# ---- through the loss --------------------------------------------------------------------------
C_LOSS, N_LOSS = 3, 37


def observations():
    rng = np.random.default_rng(11)
    comp = rng.integers(0, C_LOSS, N_LOSS)
    x = np.array([-4.0, 0.5, 5.0])[comp] + np.array([0.6, 1.0, 1.5])[comp] * rng.normal(size=N_LOSS)
    return torch.tensor(x, dtype=torch.float32)


def clustering(device, masked=False):
    x = observations().to(device)
    if masked:
        on = torch.ones(N_LOSS, dtype=torch.bool, device=device)
        on[[3, 20]] = False
        x = x.clone()
        x[3] = float("nan")
        x = torch.masked.as_masked_tensor(x, on)
    one, zero, five = (torch.tensor(v, device=device) for v in (1.0, 0.0, 5.0))

    def model():
        w = mi.sample("w", Dirichlet(torch.ones(C_LOSS, device=device)))
        mu = mi.sample("mu", Normal(zero, five), sample_shape=[C_LOSS])
        sd = mi.sample("sd", LogNormal(zero, one), sample_shape=[C_LOSS])
        mi.sample("x", MixtureSameFamily(Categorical(probs=w), Normal(mu, sd)),
                  sample_shape=[N_LOSS])

    return mi.condition(model, x=x)


def guide(device):
    return ParameterizedFactorizedDistribution(
        w=ParameterizedDistribution(Dirichlet, concentration=torch.tensor([2.0, 3.0, 1.5])),
        mu=ParameterizedDistribution(Normal, loc=torch.tensor([-3.0, 0.0, 4.0]),
                                     scale=torch.tensor([0.5, 0.4, 0.6])),
        sd=ParameterizedDistribution(LogNormal, loc=torch.tensor([-0.2, 0.1, 0.3]),
                                     scale=torch.tensor([0.2, 0.3, 0.25]))).to(device)


def noise(K):
    gen = torch.Generator().manual_seed(K)
    g = torch.distributions.Gamma(torch.tensor([2.0, 3.0, 1.5]).double(), 1.0)
    torch.manual_seed(K)
    return {"w": g.sample((K,)).float(), "mu": torch.randn(K, C_LOSS, generator=gen),
            "sd": torch.randn(K, C_LOSS, generator=gen)}


def reference_loss(module, eps, masked):
    """The loss and its gradients in float64 torch on the host, from the same injected noise."""
    leaves, dists = {}, {}
    for name, factor in module.items():
        cls = factor.distribution_cls
        constrained = {}
        for pname, p in factor.distribution_parameters.items():
            leaf = p.detach().cpu().double().clone().requires_grad_()
            leaves[f"{name}.{pname}"] = leaf
            constrained[pname] = transform_to(cls.arg_constraints[pname])(leaf)
        dists[name] = cls(**constrained)
    # x = g / sum g at the injected Gamma variates, torch's implicit gradient attached
    w = dref.injected_draw(dists["w"].concentration, dref.normalise(eps["w"]).double())
    mu = dists["mu"].loc + dists["mu"].scale * eps["mu"].double()
    sd = (dists["sd"].loc + dists["sd"].scale * eps["sd"].double()).exp()
    x = observations().double()
    on = torch.ones(N_LOSS, dtype=torch.bool)
    if masked:
        on[[3, 20]] = False
    lik = MixtureSameFamily(Categorical(probs=w[:, None, :]), Normal(mu[:, None, :], sd[:, None, :]),
                            validate_args=False).log_prob(x)
    lp = Dirichlet(torch.ones(C_LOSS).double()).log_prob(w) + \
        Normal(0.0, 5.0).log_prob(mu).sum(-1) + LogNormal(0.0, 1.0).log_prob(sd).sum(-1) + \
        torch.where(on, lik, torch.zeros((), dtype=torch.float64)).sum(-1)
    loss = -lp.mean() - sum(d.entropy().sum() for d in dists.values())
    loss.backward()
    return float(loss), {n: leaf.grad for n, leaf in leaves.items()}


def evaluate(device, K, masked):
    module = guide(device)
    seen = []
    original = engine.plan_groups

    def spy(trace, *args, **kwargs):
        seen.append(trace)
        return original(trace, *args, **kwargs)

    engine.plan_groups = spy
    try:
        loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=5)
        eps = noise(K)
        loss = loss_fn(clustering(device, masked), module(),
                       _noise={n: t.to(device) for n, t in eps.items()})
        loss.backward()
    finally:
        engine.plan_groups = original
    grads = {f"{name}.{pname}": p.grad.detach().cpu().double()
             for name, factor in module.items()
             for pname, p in factor.distribution_parameters.items()}
    return float(loss.detach()), grads, seen[-1], module, eps


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("K", [8, 40])
def test_loss_against_float64(device, K, masked):
    loss, grads, trace, module, eps = evaluate(device, K, masked)
    assert trace.fallback == []
    assert [s.family for s in trace.sites] == ["dirichlet", "normal", "log_normal",
                                               "mixture_normal"]
    d = MixtureSameFamily(Categorical(probs=torch.ones(3) / 3), Normal(torch.zeros(3), 1.0))
    assert particles.classify(d)[0] == "mixture_normal"
    want, want_grads = reference_loss(module, eps, masked)
    err = abs(loss - want) / abs(want)
    print(f"loss {loss:.8g} reference {want:.8g}: error {err:.3g}")
    assert err <= 1e-5
    for name, got in grads.items():
        w = want_grads[name]
        e = float((got - w).abs().max()) / float(w.abs().max())
        print(f"  d{name}: error {e:.3g} of the max-norm")
        assert e <= 2e-5, name


def test_captured_step_reproduces_eager_steps(device):
    def setup():
        module = guide(device)
        optimizer = mi.optim.Adam(module.parameters(), lr=0.01)
        loss_fn = EvidenceLowerBoundLoss(num_particles=8, seed=17)
        model = clustering(device)

        def step():
            optimizer.zero_grad(set_to_none=True)
            loss = loss_fn(model, module())
            loss.backward()
            optimizer.step()
            return loss
        return step, module

    eager_step, eager_module = setup()
    eager = [float(eager_step()) for _ in range(4)]
    graph_step, graph_module = setup()
    captured = StepGraph(graph_step, warmup=2)
    replays = [float(captured()) for _ in range(2)]
    captured.check()
    torch.testing.assert_close(torch.tensor(replays), torch.tensor(eager[2:]), rtol=1e-6, atol=0)
    for a, b in zip(eager_module.parameters(), graph_module.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


# ---- predictive --------------------------------------------------------------------------------
def draw_native(device, params, S, T, B, C):
    tensors = [on_device(a, device, (S, B, C)) for a in params]
    out_flat, out = guarded((S * T * B,), device)
    strided = []
    for t in tensors:
        ss, sb, sc = t.stride()
        strided.extend((t.data_ptr(), 0 if S == 1 else ss, 0 if B == 1 else sb,
                        0 if C == 1 else sc))
    code = nat.lib().mi_predictive_mixture_normal(*strided, S, T, B, C, mref.DRAW_SEED,
                                                  mref.DRAW_STREAM, out.data_ptr(),
                                                  nat.stream_handle(device))
    assert code == 0
    torch.cuda.synchronize()
    assert bool((out_flat[-GUARD:] == SENTINEL).all())
    return out.cpu().numpy().astype(np.float64)


DRAW_WORST = [0.0, 0.0]


@pytest.mark.parametrize("C", mref.DRAW_C)
def test_predictive_draw_against_reference(device, C):
    count = total = 0
    for shared, (S, T, B, _) in itertools.product(
            (False, True), [case for case in mref.DRAW_CASES if case[3] == C]):
        params = mref.draw_parameters(S, B, C, shared)
        got = draw_native(device, params, S, T, B, C)
        want, comp, marked, size = mref.draw(*params, S, T, mref.DRAW_SEED, mref.DRAW_STREAM)
        want32, comp32, _, _ = mref.draw(*params, S, T, mref.DRAW_SEED, mref.DRAW_STREAM, np.float32)
        count, total = count + int(marked.sum()), total + marked.size
        # given the component, the value is loc_c + scale_c eps: a draw of another component
        # misses by the distance between two components, far beyond the bound
        frac = np.abs(got - want) / size
        keep = ~marked
        theirs = np.abs(want32 - want)[keep & (comp32 == comp)] / size[keep & (comp32 == comp)]
        DRAW_WORST[0] = max(DRAW_WORST[0], float(frac[keep].max(initial=0.0)))
        DRAW_WORST[1] = max(DRAW_WORST[1], float(theirs.max(initial=0.0)))
        print(f"S={S} T={T} B={B} C={C} shared={shared}: value {frac[keep].max(initial=0.0):.3g} "
              f"(float32 restatement {theirs.max(initial=0.0):.3g}); largest so far {DRAW_WORST}")
        assert np.all(frac[keep] <= BOUND["draw"]), (S, T, B, C)
    assert count <= 0.01 * total


def predictive_model(device, n=6):
    def model():
        w = mi.sample("w", Dirichlet(torch.ones(C_LOSS, device=device)))
        mu = mi.sample("mu", Normal(torch.zeros((), device=device), 5.0), sample_shape=[C_LOSS])
        sd = mi.sample("sd", LogNormal(torch.zeros((), device=device), 1.0),
                       sample_shape=[C_LOSS])
        mi.sample("x", MixtureSameFamily(Categorical(probs=w), Normal(mu, sd)), sample_shape=[n])
    return model


def posterior(device, S):
    gen = torch.Generator().manual_seed(3)
    w = torch.distributions.Dirichlet(torch.ones(C_LOSS)).sample((S,))
    return {"w": w.to(device), "mu": (3 * torch.randn(S, C_LOSS, generator=gen)).to(device),
            "sd": torch.rand(S, C_LOSS, generator=gen).add(0.3).to(device)}


def test_broadcast_samples_draws_the_mixture_natively(device):
    S, n = 33, 6
    states = posterior(device, S)
    predictive.reset_counts()
    torch.manual_seed(1)
    first = mi.broadcast_samples(predictive_model(device, n), states)["x"]
    assert predictive.native_draws() == {"MixtureSameFamily": 1}
    assert first.shape == (S, n) and first.dtype == torch.float32 and first.device.type == "cuda"
    torch.manual_seed(1)
    again = mi.broadcast_samples(predictive_model(device, n), states)["x"]
    assert torch.equal(first, again)
    torch.manual_seed(2)
    other = mi.broadcast_samples(predictive_model(device, n), states)["x"]
    assert not torch.equal(first, other)
    # the first 17 samples alone are rows 0-16 of the full run
    torch.manual_seed(1)
    head = mi.broadcast_samples(predictive_model(device, n),
                                {k: v[:17] for k, v in states.items()})["x"]
    assert torch.equal(head, first[:17])
    # every value lies where its mixture puts mass: within 8 scales of some component
    z = (first[:, :, None] - states["mu"][:, None, :]).abs() / states["sd"][:, None, :]
    assert bool((z.min(-1).values < 8).all())
