"""
A random-intercept model end to end on the gathered site (N = 500, G = 12, K = 8, Normal guides):
``y ~ Normal(alpha[group], sigma)`` and ``c ~ Poisson((a + b * alpha[group]).exp())``. The fused
step equals the step with MININF_AMD_DEFER_GATHER=0 (the model's own gather and torch's
scatter-add backward), runs both sites on mi_gather_site_forward, calls no gather on a batched
tensor, has no index node in its autograd graph, is bit-identical from one evaluation to the next
and from a captured replay to the eager step; LogLikelihoodLoss (one particle) matches torch.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Normal, Poisson

import mininf_amd as mi

pytestmark = pytest.mark.gpu

N, G, K = 500, 12, 8


def index_nodes(tensor):
    """Names of the autograd nodes behind ``tensor`` that gather or scatter along an index."""
    seen, stack, found = set(), [tensor.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        # torch's own nodes: IndexBackward0, IndexPutBackward0, IndexSelectBackward0,
        # GatherBackward0, ScatterAddBackward0, TakeBackward0 (not this package's functions)
        if name.startswith(("Index", "Gather", "Scatter", "Take")):
            found.append(name)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return found


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(5)
    group = rng.integers(0, G, N)
    group[:G] = np.arange(G)
    alpha = rng.normal(0, 0.8, G)
    y = (alpha[group] + 0.5 * rng.normal(size=N)).astype(np.float32)
    c = rng.poisson(np.exp(0.3 + 0.6 * alpha[group])).astype(np.float32)
    shapes = {"alpha": (G,), "log_sigma": (), "a": (), "b": ()}
    guides = {name: ((0.2 * rng.normal(size=shape)).astype(np.float32),
                     np.exp(-1.5 + 0.1 * rng.normal(size=shape)).astype(np.float32))
              for name, shape in shapes.items()}
    eps = {name: rng.normal(size=(K,) + shape).astype(np.float32) for name, shape in shapes.items()}
    return dict(group=group, y=y, c=c, guides=guides, eps=eps)


def make_model(group):
    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        sigma = mi.sample("log_sigma", Normal(0, 1)).exp()
        a = mi.sample("a", Normal(0, 1))
        b = mi.sample("b", Normal(0, 1))
        mi.sample("y", Normal(alpha[group], sigma))
        mi.sample("c", Poisson((a + b * alpha[group]).exp()))
    return model


class GatherSpy(torch.overrides.TorchFunctionMode):
    NAMES = ("__getitem__", "index_select", "gather", "index_put", "index_put_", "index_add",
             "index_add_", "scatter_add", "scatter_add_")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in self.NAMES and args and \
                isinstance(args[0], torch.Tensor) and torch._C._functorch.is_batchedtensor(args[0]):
            self.seen.append(func.__name__)
        return func(*args, **(kwargs or {}))


def step(problem, group=None, y=None):
    device = torch.device("cuda")
    group = torch.as_tensor(problem["group"] if group is None else group, device=device)
    data = {"y": torch.as_tensor(problem["y"] if y is None else y, device=device),
            "c": torch.as_tensor(problem["c"], device=device)}
    guides = {name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                    scale=torch.as_tensor(scale)).to(device)
              for name, (loc, scale) in problem["guides"].items()}
    noise = {name: torch.as_tensor(e, device=device) for name, e in problem["eps"].items()}
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K)
    with GatherSpy() as spy:
        loss = loss_fn(mi.condition(make_model(group), **data),
                       {name: g() for name, g in guides.items()}, _noise=noise)
        fusions = dict(loss_fn.last_fusions)
        nodes = index_nodes(loss)   # (the backward itself runs in C++: no mode sees it)
        loss.backward()
        value = loss.detach().cpu().numpy().copy()
    grads = {f"{name}.{p}": t.grad.detach().cpu().numpy().copy()
             for name, g in guides.items() for p, t in g.distribution_parameters.items()}
    return value, grads, fusions, spy.seen, nodes


def test_fused_step_equals_the_materialised_one(problem, monkeypatch):
    loss, grads, fusions, seen, nodes = step(problem)
    assert fusions["gathered_sites"] == 2, fusions
    assert seen == [] and nodes == [], (seen, nodes)
    monkeypatch.setenv("MININF_AMD_DEFER_GATHER", "0")
    ref_loss, ref_grads, ref_fusions, ref_seen, ref_nodes = step(problem)
    assert ref_fusions["gathered_sites"] == 0 and "__getitem__" in ref_seen
    assert ref_nodes, "the materialised step's graph has torch's index backward"
    print("GROUPED", float(loss), float(ref_loss))
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    for name, want in ref_grads.items():
        tol = 1e-5 * np.abs(want).max()
        err = np.abs(grads[name].astype(np.float64) - want).max()
        print(name, err, tol)
        assert err <= tol, (name, err, tol)


def test_two_evaluations_are_bit_identical(problem):
    first = step(problem)
    second = step(problem)
    assert first[0].tobytes() == second[0].tobytes()
    for name in first[1]:
        assert first[1][name].tobytes() == second[1][name].tobytes(), name


def test_value_outside_the_support_raises_the_reference_message(problem):
    y = problem["y"].copy()
    y[17] = np.nan
    with pytest.raises(ValueError, match="Parameter 'y' is not in the support of Normal"):
        step(problem, y=y)


def test_group_index_out_of_range_declines_on_the_host(problem):
    from mininf_amd.engine import gather
    group = problem["group"].copy()
    group[3] = G
    assert gather.index_plan(torch.as_tensor(group, device="cuda"), G) is None
    launched = []
    real = gather._GatherLauncher.run
    gather._GatherLauncher.run = lambda self, *a, **k: launched.append(1) or real(self, *a, **k)
    try:
        with pytest.raises(IndexError, match="index out of range"):
            step(problem, group=group)
    finally:
        gather._GatherLauncher.run = real
    assert launched == []


def test_replayed_step_equals_the_eager_one_bit_for_bit(problem):
    from mininf_amd.graph import StepGraph
    device = torch.device("cuda")

    def setup():
        group = torch.as_tensor(problem["group"], device=device)
        data = {"y": torch.as_tensor(problem["y"], device=device),
                "c": torch.as_tensor(problem["c"], device=device)}
        guides = torch.nn.ModuleDict({
            name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                  scale=torch.as_tensor(scale))
            for name, (loc, scale) in problem["guides"].items()}).to(device)
        optimizer = torch.optim.Adam(guides.parameters(), lr=0.02, capturable=True)
        loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=7)
        conditioned = mi.condition(make_model(group), **data)

        def body():
            optimizer.zero_grad(set_to_none=True)
            loss = loss_fn(conditioned, {name: g() for name, g in guides.items()})
            body.fusions = dict(loss_fn.last_fusions)
            loss.backward()
            optimizer.step()
            return loss
        return body, guides

    eager_step, eager_guides = setup()
    graph_body, graph_guides = setup()
    eager = [float(eager_step().detach()) for _ in range(5)]
    captured = StepGraph(graph_body, warmup=3)   # steps 0-2 eager, the replays run steps 3 and 4
    assert graph_body.fusions["gathered_sites"] == 2, graph_body.fusions   # (the captured trace)
    replayed = [float(captured().detach()) for _ in range(2)]
    captured.check()
    assert replayed == eager[3:], (replayed, eager[3:])
    for a, b in zip(eager_guides.parameters(), graph_guides.parameters()):
        assert torch.equal(a, b)


def test_log_likelihood_loss_matches_torch(problem):
    device = torch.device("cuda")
    rng = np.random.default_rng(9)
    state = {"alpha": rng.normal(0, 0.8, G), "log_sigma": np.float64(-0.4), "a": np.float64(0.3),
             "b": np.float64(0.7)}
    params = {name: torch.tensor(np.asarray(v, np.float32), device=device, requires_grad=True)
              for name, v in state.items()}
    group = torch.as_tensor(problem["group"], device=device)
    data = {"y": torch.as_tensor(problem["y"], device=device),
            "c": torch.as_tensor(problem["c"], device=device)}
    launches = []
    from mininf_amd.engine import gather
    real = gather._GatherLauncher.run
    gather._GatherLauncher.run = lambda self, *a, **k: launches.append(self.K) or real(self, *a, **k)
    try:
        with GatherSpy() as spy:
            loss = mi.nn.LogLikelihoodLoss()(mi.condition(make_model(group), **data), params)
            nodes = index_nodes(loss)
            loss.backward()
    finally:
        gather._GatherLauncher.run = real
    assert launches == [1, 1] and spy.seen == [] and nodes == [], (launches, spy.seen, nodes)
    ref = {name: torch.tensor(np.asarray(v, np.float32).astype(np.float64), requires_grad=True)
           for name, v in state.items()}
    g64 = torch.as_tensor(problem["group"])
    eta = ref["alpha"][g64]
    want = -(Normal(eta, ref["log_sigma"].exp()).log_prob(torch.as_tensor(problem["y"]).double()).sum() +
             Poisson((ref["a"] + ref["b"] * eta).exp()).log_prob(
                 torch.as_tensor(problem["c"]).double()).sum() +
             sum(Normal(0.0, 1.0).log_prob(t).sum() for t in ref.values()))
    want.backward()
    print("LLL", float(loss), float(want))
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    # the kernel tests' bound: 1e-5 of the sum of the absolute terms of each gradient
    with torch.no_grad():
        sigma2 = (2 * ref["log_sigma"]).exp()
        dy = (torch.as_tensor(problem["y"]).double() - eta) / sigma2
        dc = torch.as_tensor(problem["c"]).double() - (ref["a"] + ref["b"] * eta).exp()
        onehot = torch.nn.functional.one_hot(g64, G).double()
        bound = {"alpha": (dy.abs() + (ref["b"] * dc).abs()) @ onehot + ref["alpha"].abs(),
                 "log_sigma": (dy * dy * sigma2 - 1).abs().sum() + ref["log_sigma"].abs(),
                 "a": dc.abs().sum() + ref["a"].abs(),
                 "b": (dc * eta).abs().sum() + ref["b"].abs()}
    for name, t in ref.items():
        err = (params[name].grad.double().cpu() - t.grad).abs()
        tol = 1e-5 * bound[name] + 1e-7
        print(name, float((err / tol).max()))
        assert bool((err <= tol).all()), (name, float((err / tol).max()))
