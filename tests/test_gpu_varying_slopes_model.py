"""
A varying-slope regression end to end on the gathered slopes site (N = 500, G = 12, P = 3, K = 8,
mean-field Normal guides): ``y ~ Normal(alpha[county] + beta[county] * floor, sigma)``,
``c ~ Poisson((a + alpha[g] + beta[g] * x + gamma[g] * w + X @ theta).exp())`` and
``z ~ Bernoulli(logits=x * beta[g] + alpha[g])``. The fused step equals the step with
MININF_AMD_DEFER_SLOPE=0 (the model's own gathers and products, torch's scatter-adds in the
backward), runs the three sites on mi_gather_slopes_forward, calls no gather or product and no
[K, N] multiplication on a batched tensor, has no index, scatter or matmul node and no [K, N]
multiplication node in its autograd graph, is bit-identical from one evaluation to the next and from
a captured replay to the eager step; LogLikelihoodLoss (one particle) matches fp64 torch.

Largest fractions of the tolerances measured on an MI355X: fused against materialised step, loss
0.0 (the same float) and gradients 0.098 (theta.scale); LogLikelihoodLoss against fp64 torch, loss
0.006 and gradients 0.0083 (beta) of their bounds.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Normal, Poisson

import mininf_amd as mi
from tests.test_gpu_multilevel_model import graph_nodes

pytestmark = pytest.mark.gpu

N, G, P, K = 500, 12, 3, 8
TABLES = ("alpha", "beta", "gamma")


def mul_nodes(tensor):
    """torch's own multiplication nodes behind ``tensor`` that saved a [K, N] operand."""
    seen, stack, found = set(), [tensor.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__.startswith("Mul"):
            for name in ("_saved_self", "_saved_other"):
                saved = getattr(fn, name, None)
                if isinstance(saved, torch.Tensor) and tuple(saved.shape[-2:]) == (K, N):
                    found.append(type(fn).__name__)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return found


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(6)
    group = rng.integers(0, G, N)
    group[:G] = np.arange(G)
    alpha, beta, gamma = (rng.normal(0, s, G) for s in (0.8, 0.5, 0.3))
    X = rng.normal(size=(N, P)).astype(np.float32)
    x = (rng.random(N) < 0.4).astype(np.float32)   # (the radon model's floor indicator)
    w = rng.normal(size=N).astype(np.float32)
    eta = alpha[group] + beta[group] * x
    full = eta + gamma[group] * w + X @ rng.normal(0, 0.5 / np.sqrt(P), P)
    y = (eta + 0.5 * rng.normal(size=N)).astype(np.float32)
    c = rng.poisson(np.exp(0.3 + full)).astype(np.float32)
    z = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(np.float32)
    shapes = {"alpha": (G,), "beta": (G,), "gamma": (G,), "theta": (P,), "log_sigma": (), "a": ()}
    guides = {name: ((0.2 * rng.normal(size=shape)).astype(np.float32),
                     np.exp(-1.5 + 0.1 * rng.normal(size=shape)).astype(np.float32))
              for name, shape in shapes.items()}
    eps = {name: rng.normal(size=(K,) + shape).astype(np.float32) for name, shape in shapes.items()}
    return dict(group=group, X=X, x=x, w=w, y=y, c=c, z=z, guides=guides, eps=eps)


def make_model(g, X, x, w):
    def model():
        alpha, beta, gamma = (mi.sample(name, Normal(0, 1), sample_shape=(G,)) for name in TABLES)
        theta = mi.sample("theta", Normal(0, 1), sample_shape=(P,))
        sigma = mi.sample("log_sigma", Normal(0, 1)).exp()
        a = mi.sample("a", Normal(0, 1))
        mi.sample("y", Normal(alpha[g] + beta[g] * x, sigma))
        mi.sample("c", Poisson((a + alpha[g] + beta[g] * x + gamma[g] * w + X @ theta).exp()))
        mi.sample("z", Bernoulli(logits=x * beta[g] + alpha[g]))
    return model


class Spy(torch.overrides.TorchFunctionMode):
    """Gathers, scatters and products on a batched tensor, and multiplications of a batched [N]
    tensor (under the particle vmap: a [K, N] product)."""
    NAMES = ("__getitem__", "index_select", "gather", "index_put", "index_put_", "index_add",
             "index_add_", "scatter_add", "scatter_add_", "matmul", "__matmul__", "mv", "mm")
    MULS = ("mul", "__mul__", "__rmul__")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", "")
        batched = [a for a in args if isinstance(a, torch.Tensor) and
                   torch._C._functorch.is_batchedtensor(a)]
        if batched and (name in self.NAMES or
                        (name in self.MULS and any(tuple(a.shape) == (N,) for a in batched))):
            self.seen.append(name)
        return func(*args, **(kwargs or {}))


def _operands(problem, device):
    model = make_model(*(torch.as_tensor(problem[k], device=device) for k in ("group", "X", "x", "w")))
    return mi.condition(model, **{k: torch.as_tensor(problem[k], device=device) for k in "ycz"})


def step(problem):
    device = torch.device("cuda")
    guides = {name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                    scale=torch.as_tensor(scale)).to(device)
              for name, (loc, scale) in problem["guides"].items()}
    noise = {name: torch.as_tensor(e, device=device) for name, e in problem["eps"].items()}
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K)
    with Spy() as spy:
        loss = loss_fn(_operands(problem, device), {name: g() for name, g in guides.items()},
                       _noise=noise)
        fusions = dict(loss_fn.last_fusions)
        nodes = graph_nodes(loss) + mul_nodes(loss)   # (the backward itself runs in C++)
        loss.backward()
        value = loss.detach().cpu().numpy().copy()
    grads = {f"{name}.{p}": t.grad.detach().cpu().numpy().copy()
             for name, g in guides.items() for p, t in g.distribution_parameters.items()}
    return value, grads, fusions, spy.seen, nodes


def test_fused_step_equals_the_materialised_one(problem, monkeypatch):
    loss, grads, fusions, seen, nodes = step(problem)
    assert fusions["gathered_slope_sites"] == 3 and fusions["gathered_sites"] == 3, fusions
    assert fusions["gathered_linear_sites"] == 1, fusions   # (those with an X @ theta term)
    assert seen == [] and nodes == [], (seen, nodes)
    monkeypatch.setenv("MININF_AMD_DEFER_SLOPE", "0")
    ref_loss, ref_grads, ref_fusions, ref_seen, ref_nodes = step(problem)
    assert ref_fusions["gathered_slope_sites"] == 0 and ref_fusions["gathered_sites"] == 0
    assert "__getitem__" in ref_seen and ref_nodes
    worst = abs(float(loss) - float(ref_loss)) / (1e-5 * abs(float(ref_loss)))
    print("SLOPES loss", float(loss), float(ref_loss), worst)
    assert worst <= 1.0
    for name, want in ref_grads.items():
        tol = 1e-5 * np.abs(want).max()
        err = np.abs(grads[name].astype(np.float64) - want).max()
        print("SLOPES", name, err / tol)
        assert err <= tol, (name, err, tol)


def test_two_evaluations_are_bit_identical(problem):
    first = step(problem)
    second = step(problem)
    assert first[0].tobytes() == second[0].tobytes()
    for name in first[1]:
        assert first[1][name].tobytes() == second[1][name].tobytes(), name


def test_replayed_step_equals_the_eager_one_bit_for_bit(problem):
    from mininf_amd.graph import StepGraph
    device = torch.device("cuda")

    def setup():
        guides = torch.nn.ModuleDict({
            name: mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(loc),
                                                  scale=torch.as_tensor(scale))
            for name, (loc, scale) in problem["guides"].items()}).to(device)
        optimizer = torch.optim.Adam(guides.parameters(), lr=0.02, capturable=True)
        loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=7)
        conditioned = _operands(problem, device)

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
    assert graph_body.fusions["gathered_slope_sites"] == 3, graph_body.fusions
    replayed = [float(captured().detach()) for _ in range(2)]
    captured.check()
    assert replayed == eager[3:], (replayed, eager[3:])
    for a, b in zip(eager_guides.parameters(), graph_guides.parameters()):
        assert torch.equal(a, b)


def test_log_likelihood_loss_matches_torch(problem):
    device = torch.device("cuda")
    rng = np.random.default_rng(9)
    state = {"alpha": rng.normal(0, 0.8, G), "beta": rng.normal(0, 0.5, G),
             "gamma": rng.normal(0, 0.3, G), "theta": rng.normal(0, 0.3, P),
             "log_sigma": np.float64(-0.4), "a": np.float64(0.3)}
    params = {name: torch.tensor(np.asarray(v, np.float32), device=device, requires_grad=True)
              for name, v in state.items()}
    launches = []
    from mininf_amd.engine import gather
    real = gather._GatherLauncher.run
    gather._GatherLauncher.run = \
        lambda self, *a, **k: launches.append((self.K, self.slopes)) or real(self, *a, **k)
    try:
        with Spy() as spy:
            loss = mi.nn.LogLikelihoodLoss()(_operands(problem, device), params)
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
    x, w, y, c, z = (torch.as_tensor(problem[k]).double() for k in ("x", "w", "y", "c", "z"))
    eta = ref["alpha"][g64] + ref["beta"][g64] * x
    full = ref["a"] + eta + ref["gamma"][g64] * w + X64 @ ref["theta"]
    want = -(Normal(eta, ref["log_sigma"].exp()).log_prob(y).sum() +
             Poisson(full.exp()).log_prob(c).sum() +
             Bernoulli(logits=eta).log_prob(z).sum() +
             sum(Normal(0.0, 1.0).log_prob(t).sum() for t in ref.values()))
    want.backward()
    got, want = float(loss.detach()), float(want.detach())
    print("LLL", got, want)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    # the kernel tests' bound: 1e-5 of the sum of the absolute terms of each gradient
    with torch.no_grad():
        sigma2 = (2 * ref["log_sigma"]).exp()
        dy = (y - eta) / sigma2
        dc = c - full.exp()
        dz = z - torch.sigmoid(eta)
        rows = dy.abs() + dc.abs() + dz.abs()
        onehot = torch.nn.functional.one_hot(g64, G).double()
        bound = {"alpha": rows @ onehot + ref["alpha"].abs(),
                 "beta": (rows * x.abs()) @ onehot + ref["beta"].abs(),
                 "gamma": (dc.abs() * w.abs()) @ onehot + ref["gamma"].abs(),
                 "theta": dc.abs() @ X64.abs() + ref["theta"].abs(),
                 "log_sigma": (dy * dy * sigma2 - 1).abs().sum() + ref["log_sigma"].abs(),
                 "a": dc.abs().sum() + ref["a"].abs()}
    for name, t in ref.items():
        err = (params[name].grad.double().cpu() - t.grad).abs()
        tol = 1e-5 * bound[name] + 1e-7
        print("LLL", name, float((err / tol).max()))
        assert bool((err <= tol).all()), (name, float((err / tol).max()))
