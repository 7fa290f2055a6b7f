"""
Count regressions end to end on the fused linear site (N = 4096, P = 8, K = 64): a Poisson
regression through EvidenceLowerBoundLoss, on the whole data under batch(N) and on a
DeviceDataLoader minibatch, against a float64 restatement fed the same injected noise (loss and the
gradients of the guide's loc and log-scale at the north-star 1e-5); the launches fused are those of
the same model with a Normal likelihood and nothing falls back to torch. One Adam step of the
Binomial model through mininf_amd.optim.Adam (asserted to run in the held launch). A Binomial model
whose trials are a column of the same DeviceDataLoader reads them through the batch's rows; trials
that are no column of the loader keep the site off the loader's rows, with the same numbers.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Binomial, Normal, Poisson

import mininf_amd as mi
from mininf_amd import particles

pytestmark = pytest.mark.gpu

N, P, K, B = 4096, 8, 64, 1024


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(11)
    X = rng.normal(size=(N, P)).astype(np.float32)
    X[:, 0] = 1.0                                   # the intercept is a column of X
    beta = (0.3 * rng.normal(size=P)).astype(np.float32)
    eta = X.astype(np.float64) @ beta
    y = rng.poisson(np.exp(eta)).astype(np.float32)
    trials = rng.integers(1, 15, size=N).astype(np.float32)
    successes = rng.binomial(trials.astype(np.int64), 1 / (1 + np.exp(-eta))).astype(np.float32)
    loc = (0.05 * rng.normal(size=P)).astype(np.float32)
    scale = np.exp(-2.0 + 0.1 * rng.normal(size=P)).astype(np.float32)
    eps = rng.normal(size=(K, P)).astype(np.float32)
    return dict(X=X, y=y, trials=trials, successes=successes, loc=loc, scale=scale, eps=eps)


def make_model(kind, n, trials=None):
    def model():
        theta = mi.sample("theta", Normal(0, 1), sample_shape=P)
        with mi.batch(N):
            with mi.no_log_prob():
                Xs = mi.sample("X", Normal(0, 1), sample_shape=(n, P))
            if kind == "poisson":
                mi.sample("y", Poisson((Xs @ theta).exp()))
            elif kind == "normal":
                mi.sample("y", Normal(Xs @ theta, 1))
            else:
                mi.sample("y", Binomial(trials, logits=Xs @ theta))
    return model


def restatement(kind, X, y, loc, scale, eps, data_scale, trials=None):
    """loss and its gradients for loc and log-scale in float64 (torch autograd on the host)."""
    loc = torch.tensor(loc, dtype=torch.float64, requires_grad=True)
    u = torch.tensor(np.log(scale.astype(np.float64)), requires_grad=True)
    theta = loc + torch.tensor(eps, dtype=torch.float64) * u.exp()
    eta = theta @ torch.tensor(X, dtype=torch.float64).T
    yt = torch.tensor(y, dtype=torch.float64)
    one, zero = torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    if kind == "poisson":
        lik = Poisson(eta.exp()).log_prob(yt)
    else:
        lik = Binomial(torch.tensor(trials, dtype=torch.float64), logits=eta).log_prob(yt)
    joint = data_scale * lik.sum(1) + Normal(zero, one).log_prob(theta).sum(1)
    elbo = joint.mean() + Normal(loc, u.exp()).entropy().sum()
    loss = -elbo
    loss.backward()
    return float(loss), loc.grad.numpy(), u.grad.numpy()


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = 1e-5 * np.abs(want).max()
    assert np.abs(got - want).max() <= tol, (what, np.abs(got - want).max(), tol)


def drawn_eps(seed, step=0):
    """The normals the guide draws for (seed, step) on stream 0, from the oracle's generator."""
    from oracle import build as oracle_build
    eps = np.empty((K, P), np.float32)
    oracle_build.load().oracle_guide_normals(K, P, seed, step, 0, 0, eps.ctypes.data)
    return eps


def guide_of(problem, device):
    return mi.nn.ParameterizedDistribution(Normal, loc=torch.as_tensor(problem["loc"]),
                                           scale=torch.as_tensor(problem["scale"])).to(device)


def fused_loss(kind, problem, device, minibatch):
    from mininf_amd.data import DeviceDataLoader
    X = torch.as_tensor(problem["X"], device=device)
    y = torch.as_tensor(problem["y"], device=device)
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
        loss = loss_fn(mi.condition(make_model(kind, n), X=Xb, y=yb), {"theta": guide()},
                       _noise={"theta": torch.as_tensor(problem["eps"], device=device)})
        loss.backward()
    finally:
        particles.trace_particles = real
    return float(loss), guide.distribution_parameters, dict(loss_fn.last_fusions), traces


@pytest.mark.parametrize("minibatch", [False, True], ids=["batch_N", "loader"])
def test_poisson_regression_against_float64(problem, device, minibatch):
    loss, params, fusions, traces = fused_loss("poisson", problem, device, minibatch)
    n = B if minibatch else N
    ref = restatement("poisson", problem["X"][:n], problem["y"][:n], problem["loc"],
                      problem["scale"], problem["eps"], N / n)
    print("POISSON", minibatch, loss, ref[0], fusions)
    assert abs(loss - ref[0]) <= 1e-5 * abs(ref[0]), (loss, ref[0])
    close(params["loc"].grad.cpu(), ref[1], "grad loc")
    close(params["scale"].grad.cpu(), ref[2], "grad log-scale")
    for t in traces:
        assert t.fallback == []
    _, _, normal_fusions, _ = fused_loss("normal", problem, device, minibatch)
    assert fusions == normal_fusions, (fusions, normal_fusions)


def test_binomial_regression_adam_step(problem, device):
    from mininf_amd.optim import Adam
    X = torch.as_tensor(problem["X"], device=device)
    y = torch.as_tensor(problem["successes"], device=device)
    trials = torch.as_tensor(problem["trials"], device=device)
    guide = guide_of(problem, device)
    lr = 0.01
    optimizer = Adam(guide.parameters(), lr=lr)
    # nothing injected: theta is drawn by the linear launch, whose normals the oracle reproduces
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=5)
    eps = drawn_eps(5)
    optimizer.zero_grad(set_to_none=True)
    loss = loss_fn(mi.condition(make_model("binomial", N, trials), X=X, y=y), {"theta": guide()})
    loss.backward()
    optimizer.step()
    # the held launch: the ELBO forward wrote the final gradients and Adam ran in its last block
    fusions = dict(loss_fn.last_fusions)
    print("BINOMIAL ADAM", fusions)
    assert fusions["final_grads"] == 1 and fusions["optimizer_step"] == 1, fusions
    value = float(loss)
    ref = restatement("binomial", problem["X"], problem["successes"], problem["loc"],
                      problem["scale"], eps, 1.0, trials=problem["trials"])
    assert abs(value - ref[0]) <= 1e-5 * abs(ref[0]), (value, ref[0])
    # Adam's first step moves every element by lr against the sign of its gradient
    # (|g| / (|g| + 1e-8), |g| >> 1e-8 here)
    assert np.abs(ref[1]).min() > 1e-3 and np.abs(ref[2]).min() > 1e-3
    # (each parameter is a float32 of magnitude below 4: the step lands within one ulp of it)
    params = guide.distribution_parameters
    for name, start, grad in (("loc", problem["loc"], ref[1]),
                              ("scale", np.log(problem["scale"]), ref[2])):
        got = params[name].detach().cpu().numpy().astype(np.float64)
        want = start.astype(np.float64) - lr * np.sign(grad)
        assert np.abs(start).max() < 4.0
        assert np.abs(got - want).max() <= 1e-5 * lr + 2.0 ** -22, (name, got, want)


@pytest.mark.parametrize("column", [True, False], ids=["loader_column", "outside_tensor"])
def test_binomial_minibatch_reads_the_count_with_the_rows(problem, device, column, monkeypatch):
    from mininf_amd.data import DeviceDataLoader
    from mininf_amd.engine import _LinearLauncher
    launches = []
    real_run = _LinearLauncher.run

    def spy_run(self, *args, **kwargs):
        launches.append((self.batch is not None, self.count_src is not None))
        return real_run(self, *args, **kwargs)
    monkeypatch.setattr(_LinearLauncher, "run", spy_run)
    X = torch.as_tensor(problem["X"], device=device)
    y = torch.as_tensor(problem["successes"], device=device)
    trials = torch.as_tensor(problem["trials"], device=device)
    guide = guide_of(problem, device)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=5)
    eps = drawn_eps(5)
    if column:
        loader = DeviceDataLoader(X, y, trials, batch_size=B, shuffle=False, drop_last=True, seed=0)
        Xb, yb, tb = loader.next()
    else:
        loader = DeviceDataLoader(X, y, batch_size=B, shuffle=False, drop_last=True, seed=0)
        Xb, yb = loader.next()
        tb = trials[:B].clone()      # the first batch's rows, but no column of the loader
    loss = loss_fn(mi.condition(make_model("binomial", B, tb), X=Xb, y=yb), {"theta": guide()})
    loss.backward()
    fusions = dict(loss_fn.last_fusions)
    print("BINOMIAL LOADER", column, fusions)
    # the site reads X, y and the trials through the batch's rows (the dataset columns) only when
    # the trials are a column of the same loader; otherwise it reads gathered buffers. (The
    # Binomial constructor reads its total_count, so the rows are drawn before the launch.)
    assert launches == [(column, column)], launches
    assert fusions["linear_theta_draws"] == 1 and fusions["final_grads"] == 1, fusions
    ref = restatement("binomial", problem["X"][:B], problem["successes"][:B], problem["loc"],
                      problem["scale"], eps, N / B, trials=problem["trials"][:B])
    assert abs(float(loss) - ref[0]) <= 1e-5 * abs(ref[0]), (float(loss), ref[0])
    params = guide.distribution_parameters
    close(params["loc"].grad.cpu(), ref[1], "grad loc")
    close(params["scale"].grad.cpu(), ref[2], "grad log-scale")
