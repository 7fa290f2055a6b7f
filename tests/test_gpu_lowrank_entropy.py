"""
The native LowRankMultivariateNormal entropy on the MI355X: mi_lowrank_entropy against the float64
closed form of tests/lowrank_entropy_reference.py point by point, its value-only mode, guard words
and determinism, and the entropy through EvidenceLowerBoundLoss (parity with float64 torch under
injected noise, the cut of its graph at the constructor, a user-constructed factor, a captured
training step, fallbacks).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from torch.distributions import LowRankMultivariateNormal, Normal

import mininf_amd as mi
from mininf_amd import _native as nat, guide
from mininf_amd.graph import StepGraph
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution
from tests import lowrank_entropy_reference as ref

pytestmark = pytest.mark.gpu

# the draw's shapes: both code paths (R < 32 on the VALU, R >= 32 on the matrix cores), every padded
# rank (4, 8, 16, 32), ragged row and rank tiles, more than one block of log d partials
SHAPES = ((1, 1), (3, 2), (31, 3), (32, 32), (33, 33), (130, 31), (130, 128), (1025, 4), (4100, 64))
VALUE_RTOL = 4 * 2.0 ** -24   # fp64 sums, one f32 rounding of the output (and of any hand-off)
GRAD_C = 2e-5                 # the draw's kernel tests' coefficient: 128 * 2^-24 = 7.7e-6 below it
GUARD = 16                    # guard words after every buffer the kernels write
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def case(D, R):
    """The case's float32 inputs (held in float64) and their float64 closed form, computed once."""
    W, d, L = ref.inputs(D, R, ref.case_seed(D, R))
    return (W, d, L) + ref.closed_form(W, d, L)


def guarded(device, n, dtype=torch.float32):
    """n NaN elements followed by GUARD sentinel words."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=device)
    buf[:n] = float("nan")
    return buf


def call(device, W, d, L, grads=True):
    """(H, dW, dd, buffers) of one mi_lowrank_entropy call over guarded, poisoned buffers."""
    D, R = W.shape
    W_d, d_d, L_d = (torch.as_tensor(a, dtype=torch.float32, device=device).contiguous()
                     for a in (W, d, L))
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_lowrank_entropy_workspace_bytes(D, R, ctypes.byref(size)), "workspace")
    assert size.value % 8 == 0
    ws = torch.full((size.value + 4 * GUARD,), 0x5A, dtype=torch.uint8, device=device)
    out = guarded(device, 1)
    dW = guarded(device, D * R) if grads else None
    dd = guarded(device, D) if grads else None
    nat.check(lib.mi_lowrank_entropy(
        W_d.data_ptr(), d_d.data_ptr(), L_d.data_ptr(), D, R, ws.data_ptr(), size.value,
        out.data_ptr(), nat.ptr(dW), nat.ptr(dd), None), "mi_lowrank_entropy")
    torch.cuda.synchronize()
    assert (ws[size.value:] == 0x5A).all(), "the workspace's guard bytes were written"
    for name, buf, n in (("entropy", out, 1), ("dW", dW, D * R), ("dd", dd, D)):
        if buf is not None:
            assert (buf[n:] == SENTINEL).all(), f"the guard words of {name} were written"
    return out[:1], None if dW is None else dW[:D * R].reshape(D, R), \
        None if dd is None else dd[:D]


def host64(t):
    return t.cpu().numpy().astype(np.float64)


# ---- 1. kernel level ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,R", SHAPES)
def test_value_and_gradients_match_float64(device, D, R):
    W, d, L, H64, dW64, dd64, Cinv = case(D, R)
    H, dW, dd = call(device, W, d, L)
    err_H = abs(float(H) - H64)
    bound_H = VALUE_RTOL * abs(H64)
    M = W @ Cinv
    bound_W = GRAD_C * (np.abs(W) @ np.abs(Cinv)) / d[:, None]
    bound_d = GRAD_C * (1.0 / d + np.abs(M * W).sum(1) / d ** 2)
    err_W = np.abs(host64(dW) - dW64)   # NaN (an unwritten element) fails the comparison
    err_d = np.abs(host64(dd) - dd64)
    print(f"D={D} R={R}: largest error / bound: H {err_H / bound_H:.3g} "
          f"dW {np.nanmax(err_W / bound_W):.3g} dd {np.nanmax(err_d / bound_d):.3g}")
    assert err_H <= bound_H, (float(H), H64)
    assert (err_W <= bound_W).all(), (err_W / bound_W).max()
    assert (err_d <= bound_d).all(), (err_d / bound_d).max()
    # value only: the same H bit for bit
    H_only, _, _ = call(device, W, d, L, grads=False)
    assert torch.equal(H_only, H)
    # two calls on the same inputs are bit-identical
    H2, dW2, dd2 = call(device, W, d, L)
    assert torch.equal(H2, H) and torch.equal(dW2, dW) and torch.equal(dd2, dd)


def test_only_the_lower_triangle_is_read(device):
    D, R = 33, 33
    W, d, L = case(D, R)[:3]
    H, dW, dd = call(device, W, d, L)
    poisoned = L + np.triu(np.full((R, R), np.nan), 1)
    H2, dW2, dd2 = call(device, W, d, poisoned)
    assert torch.equal(H2, H) and torch.equal(dW2, dW) and torch.equal(dd2, dd)


# ---- 2. through the loss: the regression of tests/test_gpu_lowrank_guide.py --------------------
N_ROWS, P, RANK = 96, 33, 4
NAMES = ("loc", "cov_factor", "cov_diag")


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


def initial_parameters():
    rng = np.random.default_rng(42)
    loc = rng.standard_normal(P)
    W = rng.standard_normal((P, RANK)) / math.sqrt(RANK)
    d = 0.2 + rng.random(P)
    return (torch.as_tensor(0.1 * loc, dtype=torch.float32),
            torch.as_tensor(0.2 * W, dtype=torch.float32),
            torch.as_tensor(0.1 * d, dtype=torch.float32))


def lowrank_guide(device):
    loc, W, d = initial_parameters()
    return ParameterizedDistribution(LowRankMultivariateNormal, loc=loc, cov_factor=W,
                                     cov_diag=d).to(device)


def evaluate(device, K, seed, noise, detach_tril=False):
    """Loss and unconstrained-parameter gradients of one evaluation with a fresh loss and guide."""
    module = lowrank_guide(device)
    init = {name: module.distribution_parameters[name].detach().cpu().double().clone()
            for name in NAMES}
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=seed)
    factor = module()
    if detach_tril:
        factor._capacitance_tril = factor._capacitance_tril.detach().clone()
    loss = loss_fn(regression_model(device), {"theta": factor}, _noise={"theta": noise})
    loss.backward()
    torch.cuda.synchronize()
    grads = {name: module.distribution_parameters[name].grad.detach().clone() for name in NAMES}
    return loss.detach().clone(), grads, dict(loss_fn.last_fusions), init


def reference(leaves, cov_diag, eps):
    """float64 torch on the host: the factor of the same parameters, its draws from the same eps
    (rsample's own formula), its own entropy. Returns the loss; the caller differentiates."""
    X, y = (t.double() for t in regression_data())
    factor = LowRankMultivariateNormal(leaves["loc"], leaves["cov_factor"], cov_diag)
    eps = eps.double()
    eps_D, eps_W = eps[:, :P], eps[:, P:]
    z = factor.loc + eps_W @ factor._unbroadcasted_cov_factor.T + \
        factor._unbroadcasted_cov_diag.sqrt() * eps_D
    lp = Normal(0.0, 1.0).log_prob(z).sum(-1) + Normal(z @ X.T, 0.5).log_prob(y).sum(-1)
    return -lp.mean() - factor.entropy()


def assert_table_tolerances(label, loss, grads, want, want_grads):
    """Loss within 1e-5 relative, every gradient within 2e-5 of its vector's max-norm."""
    rel = abs(float(loss) - float(want)) / abs(float(want))
    print(f"{label}: loss {float(loss):.8g} reference {float(want):.8g}: {rel / 1e-5:.3g} of the "
          "bound")
    failures = [] if rel <= 1e-5 else [("loss", rel)]
    for name in NAMES:
        ref_grad = want_grads[name]
        err = float((grads[name].cpu().double() - ref_grad).abs().max()) / \
            float(ref_grad.abs().max())
        print(f"  d{name}: {err / 2e-5:.3g} of the bound")
        if not err <= 2e-5:
            failures.append((name, err))
    assert not failures, failures


@pytest.mark.parametrize("K", (8, 40))
def test_loss_matches_float64_torch_under_injected_noise(device, K):
    eps = torch.randn(K, P + RANK, generator=torch.Generator().manual_seed(100 + K))
    loss, grads, fusions, init = evaluate(device, K, seed=21, noise=eps)
    assert fusions["lowrank_entropies"] == 1
    assert fusions["lowrank_draws"] == 1
    leaves = {name: init[name].clone().requires_grad_() for name in NAMES}
    want = reference(leaves, leaves["cov_diag"].exp(), eps)
    want.backward()
    assert_table_tolerances(f"K={K}", loss, grads, want.detach(),
                            {name: leaves[name].grad for name in NAMES})
    # the entropy's graph is cut at the constructor: with a detached clone for _capacitance_tril
    # nothing could flow through it, and nothing changes
    loss_cut, grads_cut, fusions_cut, _ = evaluate(device, K, seed=21, noise=eps, detach_tril=True)
    assert fusions_cut["lowrank_entropies"] == 1
    assert torch.equal(loss_cut, loss)
    for name in NAMES:
        assert torch.equal(grads_cut[name], grads[name]), name


def test_user_constructed_factor(device):
    """torch's own constructor on leaf tensors, passed in a dict: no ParameterizedDistribution."""
    K = 40
    eps = torch.randn(K, P + RANK, generator=torch.Generator().manual_seed(7))
    init = dict(zip(NAMES, initial_parameters()))
    init["cov_diag"] = init["cov_diag"].exp()   # the constrained value itself is the leaf
    leaves = {name: init[name].clone().to(device).requires_grad_() for name in NAMES}
    factor = LowRankMultivariateNormal(leaves["loc"], leaves["cov_factor"], leaves["cov_diag"])
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=3)
    loss = loss_fn(regression_model(device), {"theta": factor}, _noise={"theta": eps})
    loss.backward()
    torch.cuda.synchronize()
    assert loss_fn.last_fusions["lowrank_entropies"] == 1
    assert loss_fn.last_fusions["lowrank_draws"] == 1
    host = {name: init[name].double().clone().requires_grad_() for name in NAMES}
    want = reference(host, host["cov_diag"], eps)
    want.backward()
    assert_table_tolerances("user-constructed", loss.detach(),
                            {name: leaves[name].grad for name in NAMES}, want.detach(),
                            {name: host[name].grad for name in NAMES})


def test_batched_and_float64_factors_keep_the_torch_entropy(device):
    def model(shape):
        def body():
            if shape == (3,):
                # float64 draws: the site kernels refuse float64 values, so the prior is a family
                # torch evaluates, and the predictor is cast
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
        assert loss_fn.last_fusions["lowrank_entropies"] == 0
        assert guide.counts()["lowrank_entropies"] == 0
        assert torch.isfinite(loss)
        for p in module.distribution_parameters.values():
            assert p.grad is not None and torch.isfinite(p.grad).all()


# ---- 3. captured step --------------------------------------------------------------------------
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


def test_captured_step_replays_the_entropy_launches(device):
    """Nothing in the entropy depends on the host: a replay runs its three launches like any
    others, on the parameters the previous replay left."""
    eager_step, eager_module, eager_loss_fn = training_setup(device)
    eager = [float(eager_step()) for _ in range(3)]
    assert eager_loss_fn.last_fusions["lowrank_entropies"] == 1
    assert len(set(eager)) == 3
    # one eager warm-up step, then the capture of step 1 (not executed) and two replays
    graph_body, graph_module, _ = training_setup(device)
    captured = StepGraph(graph_body, warmup=1)
    replayed = [float(captured()) for _ in range(2)]
    captured.check()
    torch.testing.assert_close(torch.tensor(replayed), torch.tensor(eager[1:]), rtol=1e-6, atol=0)
    for a, b in zip(eager_module.parameters(), graph_module.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
