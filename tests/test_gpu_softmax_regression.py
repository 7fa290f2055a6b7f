"""
A multinomial logistic regression end to end on the fused softmax site (N = 300, P = 5, C = 4,
K = 8, a Normal guide over the [5, 4] coefficients): EvidenceLowerBoundLoss against the same model
with the product materialised (MININF_AMD_DEFER_MATMUL=0, the row site on X @ Theta) at 1e-5
relative, with no torch fallback, no matmul and no mi_categorical_forward in the fused step; the
same on a DeviceDataLoader batch under batch(N); a captured and replayed step against the eager
one bit for bit; a label out of range raising the reference's error; LogLikelihoodLoss at a fixed
Theta against torch.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Categorical, Normal

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd import particles

pytestmark = pytest.mark.gpu

N, P, C, K, B = 300, 5, 4, 8, 100


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(23)
    X = rng.normal(size=(N, P)).astype(np.float32)
    X[:, 0] = 1.0                                   # the intercept is a column of X
    beta = rng.normal(size=(P, C))
    y = (X @ beta + rng.gumbel(size=(N, C))).argmax(-1)
    loc = (0.1 * rng.normal(size=(P, C))).astype(np.float32)
    scale = np.exp(-1.5 + 0.1 * rng.normal(size=(P, C))).astype(np.float32)
    eps = rng.normal(size=(K, P, C)).astype(np.float32)
    return dict(X=X, y=y, loc=loc, scale=scale, eps=eps)


def make_model(n):
    def model():
        theta = mi.sample("theta", Normal(0, 1), sample_shape=(P, C))
        with mi.batch(N):
            with mi.no_log_prob():
                Xs = mi.sample("X", Normal(0, 1), sample_shape=(n, P))
            mi.sample("y", Categorical(logits=Xs @ theta))
    return model


def guide_of(problem, device):
    return mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(problem["loc"]),
                                           scale=torch.as_tensor(problem["scale"])).to(device)


class Spies:
    """Counts torch.matmul calls (a TorchFunctionMode) and mi_categorical_forward launches."""
    def __init__(self):
        self.matmuls = self.categoricals = 0

    def __enter__(self):
        spies = self

        class Mode(torch.overrides.TorchFunctionMode):
            def __torch_function__(self, func, types, args=(), kwargs=None):
                # (a matmul the deferral answers with a placeholder never gets here: the
                # DeferredMatmul mode is entered inside this one and does not call the function)
                if func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__, torch.mm,
                            torch.bmm, torch.mv, torch.einsum):
                    spies.matmuls += 1
                return func(*args, **(kwargs or {}))
        self.mode = Mode()
        self.mode.__enter__()
        lib = nat.lib()
        self.real = lib.mi_categorical_forward

        def counting(*args):
            spies.categoricals += 1
            return spies.real(*args)
        lib.mi_categorical_forward = counting
        return self

    def __exit__(self, *exc):
        nat.lib().mi_categorical_forward = self.real
        self.mode.__exit__(*exc)


def elbo_step(problem, device, minibatch, y=None):
    from mininf_amd.data import DeviceDataLoader
    X = torch.as_tensor(problem["X"], device=device)
    y = torch.as_tensor(problem["y"] if y is None else y, device=device)
    guide = guide_of(problem, device)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K)
    if minibatch:
        loader = DeviceDataLoader(X, y, batch_size=B, shuffle=False, drop_last=True, seed=0)
        Xb, yb = loader.next()
        n = B
    else:
        Xb, yb, n = X, y, N
    traces = []
    real = particles.trace_particles

    def spy(*args, **kwargs):
        traces.append(real(*args, **kwargs))
        return traces[-1]
    particles.trace_particles = spy
    try:
        with Spies() as spies:
            loss = loss_fn(mi.condition(make_model(n), X=Xb, y=yb), {"theta": guide()},
                           _noise={"theta": torch.as_tensor(problem["eps"], device=device)})
            loss.backward()
            value = float(loss)
    finally:
        particles.trace_particles = real
    params = guide.distribution_parameters
    grads = {name: p.grad.detach().cpu().numpy().astype(np.float64) for name, p in params.items()}
    return value, grads, traces, spies


def close(got, want, what):
    tol = 1e-5 * np.abs(want).max()
    assert np.abs(got - want).max() <= tol, (what, np.abs(got - want).max(), tol)


@pytest.mark.parametrize("minibatch", [False, True], ids=["batch_N", "loader"])
def test_fused_step_equals_the_materialised_one(problem, device, minibatch, monkeypatch):
    loss, grads, traces, spies = elbo_step(problem, device, minibatch)
    assert traces and all(t.fallback == [] for t in traces)
    sites = [s for t in traces for s in t.sites if s.name == "y"]
    assert sites and all(s.launcher is not None for s in sites)
    assert all((s.launcher.batch is not None) == minibatch for s in sites)
    assert spies.matmuls == 0 and spies.categoricals == 0, (spies.matmuls, spies.categoricals)
    monkeypatch.setenv("MININF_AMD_DEFER_MATMUL", "0")
    ref_loss, ref_grads, _, ref_spies = elbo_step(problem, device, minibatch)
    assert ref_spies.matmuls > 0 and ref_spies.categoricals > 0   # the spies see the other path
    print("SOFTMAX", minibatch, loss, ref_loss)
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    for name in ("loc", "scale"):
        close(grads[name], ref_grads[name], f"grad {name}")


def test_replayed_step_equals_the_eager_one_bit_for_bit(problem, device):
    from mininf_amd.graph import StepGraph

    def setup():
        X = torch.as_tensor(problem["X"], device=device)
        y = torch.as_tensor(problem["y"], device=device)
        guide = guide_of(problem, device)
        optimizer = torch.optim.Adam(guide.parameters(), lr=0.02, capturable=True)
        loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=7)
        conditioned = mi.condition(make_model(N), X=X, y=y)

        def step():
            optimizer.zero_grad(set_to_none=True)
            loss = loss_fn(conditioned, {"theta": guide()})
            loss.backward()
            optimizer.step()
            return loss
        return step, guide

    eager_step, eager_guide = setup()
    graph_body, graph_guide = setup()
    eager = [float(eager_step()) for _ in range(5)]
    captured = StepGraph(graph_body, warmup=3)   # steps 0-2 eager, the replays run steps 3 and 4
    replayed = [float(captured()) for _ in range(2)]
    captured.check()
    assert replayed == eager[3:], (replayed, eager[3:])
    for a, b in zip(eager_guide.parameters(), graph_guide.parameters()):
        assert torch.equal(a, b)


def test_label_out_of_range_raises_the_support_error(problem, device):
    y = problem["y"].copy()
    y[17] = C
    with pytest.raises(ValueError, match="is not in the support"):
        elbo_step(problem, device, False, y=y)


def test_log_likelihood_loss_matches_torch(problem, device):
    rng = np.random.default_rng(4)
    theta = torch.as_tensor(rng.normal(size=(P, C)).astype(np.float32), device=device)
    X = torch.as_tensor(problem["X"], device=device)
    y = torch.as_tensor(problem["y"], device=device)

    def model():
        th = mi.sample("theta", Normal(0, 1), sample_shape=(P, C))
        mi.sample("y", Categorical(logits=X @ th))

    with Spies() as spies:
        loss = float(mi.nn.LogLikelihoodLoss()(mi.condition(model, y=y), {"theta": theta}))
    assert spies.matmuls == 0 and spies.categoricals == 0
    t64 = theta.double().cpu()
    want = -(Categorical(logits=X.double().cpu() @ t64).log_prob(y.cpu()).sum() +
             Normal(0.0, 1.0).log_prob(t64).sum())
    assert abs(loss - float(want)) <= 1e-5 * abs(float(want)), (loss, float(want))
