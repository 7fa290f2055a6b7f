"""
The native LowRankMultivariateNormal guide factor on the MI355X: mi_lowrank_rsample and its
backward against the oracle's restatement of the Philox normals and float64 arithmetic, their
stream layout, determinism and shard invariance, and the factor through EvidenceLowerBoundLoss
(parity with float64 torch under injected noise, seeding, fallbacks, a captured training step).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from torch.distributions import LowRankMultivariateNormal, Normal

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd.graph import StepGraph
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution
from oracle import build as oracle_build

pytestmark = pytest.mark.gpu

# D % 4 != 0 padding, tile edges in D and R, the VALU (R < 32) and MFMA paths, the R cap, D beyond
# the full-rank factor's cap
SHAPES = ((1, 1), (3, 2), (31, 3), (32, 32), (33, 33), (130, 31), (130, 128), (1025, 4), (4100, 64))
KS = (1, 5, 33, 64)
SEED, STEP, STREAM, OFFSET = 1234, 3, 2, 5
NORMALS_ATOL = 2e-5   # device normals against the oracle's (test_gpu_kernels.py)
ROUNDING = 1e-5       # fp32 chain of length <= 129: 129 * 2^-24 < 1e-5


@functools.lru_cache(maxsize=None)
def oracle_lib():
    return oracle_build.load()


def oracle_eps(K, D, R, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET):
    """(eps_D [K, D], eps_W [K, R]) of the factor's stream: elements [0, D) and [Dpad, Dpad + R)."""
    dpad = 4 * ((D + 3) // 4)
    out = np.empty((K, dpad + R), np.float32)
    oracle_lib().oracle_guide_normals(K, dpad + R, seed, step, stream_id, offset, out.ctypes.data)
    out = out.astype(np.float64)
    return out[:, :D], out[:, dpad:]


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def factor(D, R, rng):
    """A random loc, cov_factor and cov_diag, as float32 values held in float64."""
    return f32(rng.standard_normal(D)), f32(rng.standard_normal((D, R)) / math.sqrt(R)), \
        f32(0.2 + rng.random(D))


def on_device(device, *arrays):
    return tuple(torch.as_tensor(a, dtype=torch.float32, device=device).contiguous() for a in arrays)


def rsample(device, loc, W, d, K, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET, eps=None,
            step_device=None):
    D, R = W.shape
    loc_d, W_d, d_d = on_device(device, loc, W, d)
    z = torch.full((K, D), float("nan"), device=device)
    nat.check(nat.lib().mi_lowrank_rsample(
        loc_d.data_ptr(), W_d.data_ptr(), d_d.data_ptr(), K, D, R, seed, step,
        nat.ptr(step_device), stream_id, offset, nat.ptr(eps), z.data_ptr(), None),
        "mi_lowrank_rsample")
    return z


def rsample_backward(device, dz, d, K, D, R, seed=SEED, step=STEP, stream_id=STREAM, offset=OFFSET,
                     eps=None, step_device=None):
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_lowrank_rsample_backward_workspace_bytes(K, D, R, ctypes.byref(size)),
              "workspace")
    ws = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    (d_d,) = on_device(device, d)
    dloc = torch.full((D,), float("nan"), device=device)
    dW = torch.full((D, R), float("nan"), device=device)
    dd = torch.full((D,), float("nan"), device=device)
    nat.check(lib.mi_lowrank_rsample_backward(
        dz.data_ptr(), dz.stride(0), dz.stride(1), d_d.data_ptr(), K, D, R, seed, step,
        nat.ptr(step_device), stream_id, offset, nat.ptr(eps), ws.data_ptr(), size.value,
        dloc.data_ptr(), dW.data_ptr(), dd.data_ptr(), None), "mi_lowrank_rsample_backward")
    return dloc, dW, dd


def host64(t):
    return t.cpu().numpy().astype(np.float64)


def forward_bound(loc, W, d, eps_D, eps_W, normals=NORMALS_ATOL):
    return normals * (np.abs(W).sum(1) + np.sqrt(d)) + \
        ROUNDING * (np.abs(loc) + np.abs(eps_W) @ np.abs(W).T + np.abs(np.sqrt(d) * eps_D))


# ---- 1. forward against the restatement --------------------------------------------------------
@pytest.mark.parametrize("D,R", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_forward_matches_restatement(device, D, R, K):
    rng = np.random.default_rng(1000 * D + 10 * R + K)
    loc, W, d = factor(D, R, rng)
    eps_D, eps_W = oracle_eps(K, D, R)
    z = rsample(device, loc, W, d, K)
    want = loc + eps_W @ W.T + np.sqrt(d) * eps_D
    bound = forward_bound(loc, W, d, eps_D, eps_W)
    err = np.abs(host64(z) - want)   # NaN (an unwritten element) fails the comparison
    print(f"D={D} R={R} K={K}: largest error / bound {np.nanmax(err / bound):.3g}")
    assert (err <= bound).all(), (err / bound).max()


# ---- 2. backward against float64 ---------------------------------------------------------------
@pytest.mark.parametrize("D,R", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_backward_matches_float64(device, D, R, K):
    rng = np.random.default_rng(7 + 1000 * D + 10 * R + K)
    _, _, d = factor(D, R, rng)
    eps_D, eps_W = oracle_eps(K, D, R)
    dz64 = f32(rng.standard_normal((K, D)))
    absdz = np.abs(dz64)
    want_loc = dz64.sum(0)
    want_W = dz64.T @ eps_W
    half = 0.5 / np.sqrt(d)
    want_d = (dz64 * eps_D).sum(0) * half
    bound_loc = ROUNDING * absdz.sum(0) + 1e-30
    bound_W = NORMALS_ATOL * absdz.sum(0)[:, None] + ROUNDING * (absdz.T @ np.abs(eps_W))
    bound_d = (NORMALS_ATOL * absdz.sum(0) + ROUNDING * (absdz * np.abs(eps_D)).sum(0)) * half
    contiguous = torch.as_tensor(dz64, dtype=torch.float32, device=device)
    transposed = contiguous.t().contiguous().t()          # strides (1, K)
    padded = torch.zeros(K, D + 3, device=device)[:, 1:D + 1]   # row stride D + 3, offset view
    padded.copy_(contiguous)
    first = None
    for dz in (contiguous, transposed, padded):
        dloc, dW, dd = rsample_backward(device, dz, d, K, D, R)
        # the kernels read the same values in the same order whatever the strides
        first = first or (dloc, dW, dd)
        assert all(torch.equal(got, ref) for got, ref in zip((dloc, dW, dd), first))
        assert (np.abs(host64(dloc) - want_loc) <= bound_loc).all()
        err_W = np.abs(host64(dW) - want_W)
        assert (err_W <= bound_W).all(), (err_W / bound_W).max()
        err_d = np.abs(host64(dd) - want_d)
        assert (err_d <= bound_d).all(), (err_d / bound_d).max()


# ---- 3. injected eps ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,R", ((3, 2), (33, 33)))
def test_parity_mode_reads_injected_eps(device, D, R):
    K = 40
    rng = np.random.default_rng(D)
    loc, W, d = factor(D, R, rng)
    eps64 = f32(rng.standard_normal((K, D + R)))
    eps_D, eps_W = eps64[:, :D], eps64[:, D:]
    eps = torch.as_tensor(eps64, dtype=torch.float32, device=device)
    z = rsample(device, loc, W, d, K, eps=eps)
    want = loc + eps_W @ W.T + np.sqrt(d) * eps_D
    bound = forward_bound(loc, W, d, eps_D, eps_W, normals=0.0)
    assert (np.abs(host64(z) - want) <= bound).all()
    # neither the seed nor the step is read
    assert torch.equal(rsample(device, loc, W, d, K, eps=eps, seed=SEED + 1, step=STEP + 1), z)
    dz64 = f32(rng.standard_normal((K, D)))
    dz = torch.as_tensor(dz64, dtype=torch.float32, device=device)
    dloc, dW, dd = rsample_backward(device, dz, d, K, D, R, eps=eps)
    absdz = np.abs(dz64)
    half = 0.5 / np.sqrt(d)
    assert (np.abs(host64(dloc) - dz64.sum(0)) <= ROUNDING * absdz.sum(0)).all()
    assert (np.abs(host64(dW) - dz64.T @ eps_W) <= ROUNDING * (absdz.T @ np.abs(eps_W))).all()
    assert (np.abs(host64(dd) - (dz64 * eps_D).sum(0) * half) <=
            ROUNDING * (absdz * np.abs(eps_D)).sum(0) * half).all()
    again = rsample_backward(device, dz, d, K, D, R, eps=eps, seed=SEED + 1, step=STEP + 1)
    for a, b in zip((dloc, dW, dd), again):
        assert torch.equal(a, b)


# ---- 4. shard invariance and determinism -------------------------------------------------------
@pytest.mark.parametrize("D,R", ((33, 33), (130, 3)))
def test_shard_invariance_and_determinism(device, D, R):
    K = 64
    rng = np.random.default_rng(5)
    loc, W, d = factor(D, R, rng)
    whole = rsample(device, loc, W, d, K, offset=0)
    first = rsample(device, loc, W, d, K // 2, offset=0)
    second = rsample(device, loc, W, d, K // 2, offset=K // 2)
    assert torch.isfinite(whole).all()
    assert torch.equal(whole[:K // 2], first)
    assert torch.equal(whole[K // 2:], second)
    # an offset that moves every particle to another row of its 32-particle tile
    shifted = rsample(device, loc, W, d, K - 7, offset=7)
    assert torch.equal(whole[7:], shifted)
    assert torch.equal(rsample(device, loc, W, d, K, offset=0), whole)
    dz = torch.as_tensor(rng.standard_normal((K, D)), dtype=torch.float32, device=device)
    one = rsample_backward(device, dz, d, K, D, R)
    two = rsample_backward(device, dz, d, K, D, R)
    for a, b in zip(one, two):
        assert torch.equal(a, b) and torch.isfinite(a).all()


# ---- 5. eps_D is the Normal factor's stream ----------------------------------------------------
@pytest.mark.parametrize("D", (33, 130))
def test_diagonal_part_matches_a_normal_factor(device, D):
    K, R = 40, 3
    rng = np.random.default_rng(11)
    loc, _, d = factor(D, R, rng)
    z = rsample(device, loc, np.zeros((D, R)), d, K)
    loc_d, d_d = on_device(device, loc, d)
    scale = d_d.sqrt()
    normal = torch.full((K, D), float("nan"), device=device)
    nat.check(nat.lib().mi_normal_rsample(
        loc_d.data_ptr(), 1, scale.data_ptr(), 1, K, D, SEED, STEP, None, STREAM, OFFSET, 0, None,
        normal.data_ptr(), None), "mi_normal_rsample")
    got, want = host64(z) - loc, host64(normal) - loc
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= 2e-7 * np.abs(want)).all()


# ---- 6. device step counter --------------------------------------------------------------------
@pytest.mark.parametrize("D,R", ((33, 33), (130, 3)))
def test_device_step_counter(device, D, R):
    """The step read from the device word (graph replays) is the same stream as the argument."""
    K = 40
    rng = np.random.default_rng(9)
    loc, W, d = factor(D, R, rng)
    counter = torch.tensor([7], dtype=torch.int64, device=device)
    by_word = rsample(device, loc, W, d, K, step=0, step_device=counter)
    by_argument = rsample(device, loc, W, d, K, step=7)
    assert torch.equal(by_word, by_argument)
    assert not torch.equal(by_word, rsample(device, loc, W, d, K, step=6))
    dz = torch.as_tensor(rng.standard_normal((K, D)), dtype=torch.float32, device=device)
    a = rsample_backward(device, dz, d, K, D, R, step=0, step_device=counter)
    b = rsample_backward(device, dz, d, K, D, R, step=7)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 7. through the loss -----------------------------------------------------------------------
N_ROWS, P, RANK = 96, 33, 4


@functools.lru_cache(maxsize=None)
def regression_data():
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(N_ROWS, P, generator=gen) / math.sqrt(P)
    y = X @ torch.randn(P, generator=gen) + 0.5 * torch.randn(N_ROWS, generator=gen)
    return X, y


def regression_model(device):
    X, y = regression_data()
    Xd = X.to(device)

    def model():
        theta = mi.sample("theta", Normal(0, 1), (P,))
        mi.sample("y", Normal(Xd @ theta, 0.5))

    return mi.condition(model, y=y.to(device))


def lowrank_guide(device):
    rng = np.random.default_rng(42)
    loc, W, d = factor(P, RANK, rng)
    return ParameterizedDistribution(
        LowRankMultivariateNormal, loc=torch.as_tensor(0.1 * loc, dtype=torch.float32),
        cov_factor=torch.as_tensor(0.2 * W, dtype=torch.float32),
        cov_diag=torch.as_tensor(0.1 * d, dtype=torch.float32)).to(device)


NAMES = ("loc", "cov_factor", "cov_diag")


def evaluate(device, K, seed, noise=None):
    """Loss and unconstrained-parameter gradients of one evaluation with a fresh loss and guide."""
    module = lowrank_guide(device)
    init = {name: module.distribution_parameters[name].detach().cpu().double().clone()
            for name in NAMES}
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=seed)
    extra = {} if noise is None else {"_noise": {"theta": noise}}
    loss = loss_fn(regression_model(device), {"theta": module()}, **extra)
    loss.backward()
    torch.cuda.synchronize()
    grads = {name: module.distribution_parameters[name].grad.detach().clone() for name in NAMES}
    return loss.detach().clone(), grads, dict(loss_fn.last_fusions), init


def reference(init, eps, dtype=torch.float64):
    """torch on the host: LowRankMultivariateNormal built from the same unconstrained parameters,
    its draws from the same eps (rsample's own formula), its own entropy."""
    X, y = (t.to(dtype) for t in regression_data())
    leaves = {name: init[name].to(dtype).clone().requires_grad_() for name in NAMES}
    factor_ = LowRankMultivariateNormal(leaves["loc"], leaves["cov_factor"],
                                        leaves["cov_diag"].exp())
    eps = eps.to(dtype)
    eps_D, eps_W = eps[:, :P], eps[:, P:]
    z = factor_.loc + eps_W @ factor_._unbroadcasted_cov_factor.T + \
        factor_._unbroadcasted_cov_diag.sqrt() * eps_D
    lp = Normal(0.0, 1.0).log_prob(z).sum(-1) + Normal(z @ X.T, 0.5).log_prob(y).sum(-1)
    loss = -lp.mean() - factor_.entropy()
    loss.backward()
    return loss.detach(), {name: leaves[name].grad for name in NAMES}


@pytest.mark.parametrize("K", (8, 40))
def test_loss_matches_float64_torch_under_injected_noise(device, K):
    """
    Injected noise, so the project's table tolerances apply unchanged: loss within 1e-5 relative,
    every guide gradient within 2e-5 of its vector's max-norm. float32 torch on the host is
    printed as the second yardstick.
    """
    eps = torch.randn(K, P + RANK, generator=torch.Generator().manual_seed(100 + K))
    loss, grads, fusions, init = evaluate(device, K, seed=21, noise=eps)
    assert fusions["lowrank_draws"] == 1
    want, want_grads = reference(init, eps)
    single, single_grads = reference(init, eps, torch.float32)
    rel = abs(float(loss) - float(want)) / abs(float(want))
    print(f"K={K}: loss {float(loss):.8g} reference {float(want):.8g}: {rel / 1e-5:.3g} of the "
          f"bound (float32 torch: {abs(float(single) - float(want)) / abs(float(want)) / 1e-5:.3g})")
    failures = [] if rel <= 1e-5 else [("loss", rel)]
    for name in NAMES:
        ref = want_grads[name]
        scale = float(ref.abs().max())
        err = float((grads[name].cpu().double() - ref).abs().max()) / scale
        host = float((single_grads[name].double() - ref).abs().max()) / scale
        print(f"  d{name}: {err / 2e-5:.3g} of the bound (float32 torch: {host / 2e-5:.3g})")
        if not err <= 2e-5:
            failures.append((name, err))
    assert not failures, failures


def test_loss_is_governed_by_its_seed(device):
    torch.manual_seed(1)
    loss_a, grads_a, fusions, _ = evaluate(device, 40, seed=21)
    assert fusions["lowrank_draws"] == 1
    torch.manual_seed(2)   # torch's generator plays no part
    loss_b, grads_b, _, _ = evaluate(device, 40, seed=21)
    assert torch.isfinite(loss_a)
    assert torch.equal(loss_a, loss_b)
    for name in NAMES:
        assert torch.equal(grads_a[name], grads_b[name]), name
    loss_c, _, _, _ = evaluate(device, 40, seed=22)
    assert not torch.equal(loss_a, loss_c)


def test_batched_and_float64_factors_fall_back(device):
    def model(shape):
        def body():
            if shape == (3,):
                # float64 draws: the site kernels compute in float32 and refuse float64 values, so
                # the prior is a family torch evaluates, and the predictor is cast
                theta = mi.sample("theta", torch.distributions.Gumbel(0.0, 1.0), shape)
            else:
                theta = mi.sample("theta", Normal(0, 1), shape)
            mi.sample("y", Normal(theta.sum().float(), 0.5))
        return body

    batched = ParameterizedDistribution(
        LowRankMultivariateNormal, loc=torch.zeros(2, 3), cov_factor=0.1 * torch.ones(2, 3, 2),
        cov_diag=0.5 * torch.ones(2, 3)).to(device)
    double = ParameterizedDistribution(
        LowRankMultivariateNormal, loc=torch.zeros(3, dtype=torch.float64),
        cov_factor=0.1 * torch.ones(3, 2, dtype=torch.float64),
        cov_diag=0.5 * torch.ones(3, dtype=torch.float64)).to(device)
    for module, shape in ((batched, (2, 3)), (double, (3,))):
        loss_fn = EvidenceLowerBoundLoss(num_particles=8, seed=1)
        loss = loss_fn(mi.condition(model(shape), y=torch.tensor(0.3, device=device)),
                       {"theta": module()})
        loss.backward()
        assert loss_fn.last_fusions["lowrank_draws"] == 0
        assert torch.isfinite(loss)
        for p in module.distribution_parameters.values():
            assert p.grad is not None and torch.isfinite(p.grad).all()


# ---- 8. captured step --------------------------------------------------------------------------
def training_setup(device):
    module = lowrank_guide(device)
    optimizer = mi.optim.Adam(module.parameters(), lr=0.01)
    loss_fn = EvidenceLowerBoundLoss(num_particles=40, seed=17)
    model = regression_model(device)

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(model, {"theta": module()})
        loss.backward()
        optimizer.step()
        return loss

    return step, module, loss_fn


def test_captured_step_draws_anew_on_every_replay(device):
    """The constructor's Cholesky runs on mi_cholesky, so the whole step can be captured."""
    eager_step, eager_module, eager_loss_fn = training_setup(device)
    eager = [float(eager_step()) for _ in range(3)]
    assert eager_loss_fn.last_fusions["lowrank_draws"] == 1
    assert len(set(eager)) == 3
    # one eager warm-up step, then the capture of step 1 (not executed) and two replays
    graph_body, graph_module, _ = training_setup(device)
    captured = StepGraph(graph_body, warmup=1)
    replayed = [float(captured()) for _ in range(2)]
    captured.check()
    torch.testing.assert_close(torch.tensor(replayed), torch.tensor(eager[1:]), rtol=1e-6, atol=0)
    for a, b in zip(eager_module.parameters(), graph_module.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
