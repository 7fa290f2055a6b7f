"""
A multilevel regression end to end on the gathered linear site (N = 500, G = 12, P = 3, K = 8,
Normal guides): ``y ~ Normal(alpha[group] + X @ theta, sigma)``,
``c ~ Poisson((a + alpha[group] + X @ theta).exp())`` and
``z ~ Bernoulli(logits=X @ theta + alpha[group])``. The fused step equals the step with
MININF_AMD_DEFER_SUM=0 (the model's own gather and product, torch's scatter-add and second
product in the backward), runs the three sites on mi_gather_linear_forward, calls no gather or
product on a batched tensor, has no index or matmul node in its autograd graph, is bit-identical
from one evaluation to the next and from a captured replay to the eager step; LogLikelihoodLoss
(one particle) matches fp64 torch; a P = 40 model takes the put-back path.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Normal, Poisson

import mininf_amd as mi

pytestmark = pytest.mark.gpu

N, G, P, K = 500, 12, 3, 8


def graph_nodes(tensor):
    """Names of torch's own autograd nodes behind ``tensor`` that gather, scatter or multiply
    matrices."""
    seen, stack, found = set(), [tensor.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        if name.startswith(("Index", "Gather", "Scatter", "Take", "Mm", "Mv", "Bmm", "Addmm")):
            found.append(name)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return found


def make_problem(p):
    rng = np.random.default_rng(5)
    group = rng.integers(0, G, N)
    group[:G] = np.arange(G)
    alpha = rng.normal(0, 0.8, G)
    X = rng.normal(size=(N, p)).astype(np.float32)
    beta = rng.normal(0, 0.5 / np.sqrt(p), p)
    eta = alpha[group] + X @ beta
    y = (eta + 0.5 * rng.normal(size=N)).astype(np.float32)
    c = rng.poisson(np.exp(0.3 + eta)).astype(np.float32)
    z = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(np.float32)
    shapes = {"alpha": (G,), "theta": (p,), "log_sigma": (), "a": ()}
    guides = {name: ((0.2 * rng.normal(size=shape)).astype(np.float32),
                     np.exp(-1.5 + 0.1 * rng.normal(size=shape)).astype(np.float32))
              for name, shape in shapes.items()}
    eps = {name: rng.normal(size=(K,) + shape).astype(np.float32) for name, shape in shapes.items()}
    return dict(group=group, X=X, y=y, c=c, z=z, guides=guides, eps=eps, p=p)


@pytest.fixture(scope="module")
def problem():
    return make_problem(P)


def make_model(group, X, p):
    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        theta = mi.sample("theta", Normal(0, 1), sample_shape=(p,))
        sigma = mi.sample("log_sigma", Normal(0, 1)).exp()
        a = mi.sample("a", Normal(0, 1))
        mi.sample("y", Normal(alpha[group] + X @ theta, sigma))
        mi.sample("c", Poisson((a + alpha[group] + X @ theta).exp()))
        mi.sample("z", Bernoulli(logits=X @ theta + alpha[group]))
    return model


class Spy(torch.overrides.TorchFunctionMode):
    NAMES = ("__getitem__", "index_select", "gather", "index_put", "index_put_", "index_add",
             "index_add_", "scatter_add", "scatter_add_", "matmul", "__matmul__", "mv", "mm")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in self.NAMES and any(
                isinstance(a, torch.Tensor) and torch._C._functorch.is_batchedtensor(a)
                for a in args):
            self.seen.append(func.__name__)
        return func(*args, **(kwargs or {}))


def _data(problem, device, y=None):
    return {"y": torch.as_tensor(problem["y"] if y is None else y, device=device),
            "c": torch.as_tensor(problem["c"], device=device),
            "z": torch.as_tensor(problem["z"], device=device)}


def step(problem, group=None, y=None):
    device = torch.device("cuda")
    group = torch.as_tensor(problem["group"] if group is None else group, device=device)
    X = torch.as_tensor(problem["X"], device=device)
    guides = {name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                    scale=torch.as_tensor(scale)).to(device)
              for name, (loc, scale) in problem["guides"].items()}
    noise = {name: torch.as_tensor(e, device=device) for name, e in problem["eps"].items()}
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K)
    with Spy() as spy:
        loss = loss_fn(mi.condition(make_model(group, X, problem["p"]), **_data(problem, device, y)),
                       {name: g() for name, g in guides.items()}, _noise=noise)
        fusions = dict(loss_fn.last_fusions)
        nodes = graph_nodes(loss)   # (the backward itself runs in C++: no mode sees it)
        loss.backward()
        value = loss.detach().cpu().numpy().copy()
    grads = {f"{name}.{p}": t.grad.detach().cpu().numpy().copy()
             for name, g in guides.items() for p, t in g.distribution_parameters.items()}
    return value, grads, fusions, spy.seen, nodes


def test_fused_step_equals_the_materialised_one(problem, monkeypatch):
    loss, grads, fusions, seen, nodes = step(problem)
    assert fusions["gathered_linear_sites"] == 3 and fusions["gathered_sites"] == 3, fusions
    assert seen == [] and nodes == [], (seen, nodes)
    monkeypatch.setenv("MININF_AMD_DEFER_SUM", "0")
    ref_loss, ref_grads, ref_fusions, ref_seen, ref_nodes = step(problem)
    assert ref_fusions["gathered_linear_sites"] == 0 and ref_fusions["gathered_sites"] == 0
    assert "__getitem__" in ref_seen and ref_nodes
    print("MULTILEVEL", float(loss), float(ref_loss))
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
    launched = []
    real = gather._GatherLauncher.run
    gather._GatherLauncher.run = lambda self, *a, **k: launched.append(1) or real(self, *a, **k)
    try:
        with pytest.raises(IndexError, match="index out of range"):
            step(problem, group=group)
    finally:
        gather._GatherLauncher.run = real
    assert launched == []


def test_wide_product_takes_the_put_back_path(monkeypatch):
    wide = make_problem(40)
    loss, grads, fusions, seen, nodes = step(wide)
    assert fusions["gathered_linear_sites"] == 0 and fusions["gathered_sites"] == 0, fusions
    monkeypatch.setenv("MININF_AMD_DEFER_SUM", "0")
    ref_loss, ref_grads, *_ = step(wide)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    for name, want in ref_grads.items():
        assert np.abs(grads[name] - want).max() <= 1e-5 * np.abs(want).max(), name


def test_replayed_step_equals_the_eager_one_bit_for_bit(problem):
    from mininf_amd.graph import StepGraph
    device = torch.device("cuda")

    def setup():
        group = torch.as_tensor(problem["group"], device=device)
        X = torch.as_tensor(problem["X"], device=device)
        guides = torch.nn.ModuleDict({
            name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                  scale=torch.as_tensor(scale))
            for name, (loc, scale) in problem["guides"].items()}).to(device)
        optimizer = torch.optim.Adam(guides.parameters(), lr=0.02, capturable=True)
        loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=7)
        conditioned = mi.condition(make_model(group, X, P), **_data(problem, device))

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
    assert graph_body.fusions["gathered_linear_sites"] == 3, graph_body.fusions
    replayed = [float(captured().detach()) for _ in range(2)]
    captured.check()
    assert replayed == eager[3:], (replayed, eager[3:])
    for a, b in zip(eager_guides.parameters(), graph_guides.parameters()):
        assert torch.equal(a, b)


def test_log_likelihood_loss_matches_torch(problem):
    device = torch.device("cuda")
    rng = np.random.default_rng(9)
    state = {"alpha": rng.normal(0, 0.8, G), "theta": rng.normal(0, 0.3, P),
             "log_sigma": np.float64(-0.4), "a": np.float64(0.3)}
    params = {name: torch.tensor(np.asarray(v, np.float32), device=device, requires_grad=True)
              for name, v in state.items()}
    group = torch.as_tensor(problem["group"], device=device)
    X = torch.as_tensor(problem["X"], device=device)
    launches = []
    from mininf_amd.engine import gather
    real = gather._GatherLauncher.run
    gather._GatherLauncher.run = \
        lambda self, *a, **k: launches.append((self.K, self.linear)) or real(self, *a, **k)
    try:
        with Spy() as spy:
            loss = mi.nn.LogLikelihoodLoss()(
                mi.condition(make_model(group, X, P), **_data(problem, device)), params)
            nodes = graph_nodes(loss)
            loss.backward()
    finally:
        gather._GatherLauncher.run = real
    assert launches == [(1, True)] * 3 and spy.seen == [] and nodes == [], \
        (launches, spy.seen, nodes)
    ref = {name: torch.tensor(np.asarray(v, np.float32).astype(np.float64), requires_grad=True)
           for name, v in state.items()}
    g64 = torch.as_tensor(problem["group"])
    X64 = torch.as_tensor(problem["X"]).double()
    y, c, z = (torch.as_tensor(problem[k]).double() for k in ("y", "c", "z"))
    eta = ref["alpha"][g64] + X64 @ ref["theta"]
    want = -(Normal(eta, ref["log_sigma"].exp()).log_prob(y).sum() +
             Poisson((ref["a"] + eta).exp()).log_prob(c).sum() +
             Bernoulli(logits=eta).log_prob(z).sum() +
             sum(Normal(0.0, 1.0).log_prob(t).sum() for t in ref.values()))
    want.backward()
    print("LLL", float(loss), float(want))
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    # the kernel tests' bound: 1e-5 of the sum of the absolute terms of each gradient
    with torch.no_grad():
        sigma2 = (2 * ref["log_sigma"]).exp()
        dy = (y - eta) / sigma2
        dc = c - (ref["a"] + eta).exp()
        dz = z - torch.sigmoid(eta)
        rows = dy.abs() + dc.abs() + dz.abs()
        onehot = torch.nn.functional.one_hot(g64, G).double()
        bound = {"alpha": rows @ onehot + ref["alpha"].abs(),
                 "theta": rows @ X64.abs() + ref["theta"].abs(),
                 "log_sigma": (dy * dy * sigma2 - 1).abs().sum() + ref["log_sigma"].abs(),
                 "a": dc.abs().sum() + ref["a"].abs()}
    for name, t in ref.items():
        err = (params[name].grad.double().cpu() - t.grad).abs()
        tol = 1e-5 * bound[name] + 1e-7
        print(name, float((err / tol).max()))
        assert bool((err <= tol).all()), (name, float((err / tol).max()))
