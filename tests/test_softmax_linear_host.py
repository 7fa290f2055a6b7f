"""
Categorical(logits = X @ Theta) on a deferred product without a GPU: the trace records the native
spellings as softmax sites without computing the product, every other spelling materialises what
torch would compute, a 1-D theta is recorded as before, the library rejects invalid arguments
before any device work, the fp64 reference of tests/softmax_linear_reference.py agrees with
torch.distributions, and a float32 restatement of the kernel's formula meets the GPU file's bounds
on every one of its input sets (the gate before any GPU time is spent).
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Categorical, Normal

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd import particles
from mininf_amd.linear import DeferredMatmul
from tests import test_gpu_softmax_linear as gpu
from tests.softmax_linear_reference import describe, float32_restatement, reference


@pytest.fixture(autouse=True)
def host_deferral(monkeypatch):
    monkeypatch.setattr(DeferredMatmul, "require_device", False)


MODES = []   # the DeferredMatmul modes of the traces of a test


@pytest.fixture(autouse=True)
def record_modes(monkeypatch):
    MODES.clear()
    init = DeferredMatmul.__init__

    def spy(self, *args, **kwargs):
        init(self, *args, **kwargs)
        MODES.append(self)
    monkeypatch.setattr(DeferredMatmul, "__init__", spy)


def products_computed():
    """The deferred products of the test's traces that something materialised."""
    infos = [info for mode in MODES for info in mode.deferred.values()]
    assert infos, "nothing was deferred"
    return [info for info in infos if info.real is not None]


N, P, C, K = 50, 3, 4, 5
X = torch.randn(N, P, generator=torch.Generator().manual_seed(1))
Y = torch.arange(N) % C


def trace(model, seed=0):
    theta = torch.randn(K, P, C, generator=torch.Generator().manual_seed(seed))
    return particles.trace_particles(model, {"theta": theta}, K), theta


def sample_theta():
    return mi.sample("theta", Normal(0.0, 1.0), sample_shape=(P, C))


@pytest.mark.parametrize("spelling,link", [
    ("logits", "log_softmax"), ("torch_log_softmax", "log_softmax"),
    ("method_log_softmax", "log_softmax"), ("functional_log_softmax", "log_softmax"),
    ("expand", "log_softmax"), ("expand_log_softmax", "log_softmax"), ("dim1", "log_softmax")])
def test_native_spellings_recorded_without_product(spelling, link):
    def model():
        eta = X @ sample_theta()
        if spelling == "torch_log_softmax":
            eta = torch.log_softmax(eta, -1)
        elif spelling == "method_log_softmax":
            eta = eta.log_softmax(dim=-1)
        elif spelling == "functional_log_softmax":
            eta = torch.nn.functional.log_softmax(eta, dim=-1)
        elif spelling == "expand":
            eta = eta.expand(N, C)
        elif spelling == "expand_log_softmax":
            eta = torch.log_softmax(eta, -1).expand(N, C)
        elif spelling == "dim1":
            eta = eta - eta.logsumexp(dim=1, keepdim=True)
        mi.sample("y", Categorical(logits=eta))

    t, theta = trace(mi.condition(model, y=Y))
    site = next(s for s in t.sites if s.name == "y")
    assert site.family == "categorical" and site.linear_X is X
    assert site.linear_link == link and site.linear_role == 0
    torch.testing.assert_close(site.linear_theta, theta)
    assert site.tensors[0].shape == (K, N, C) and site.tensors[0].stride() == (0, 0, 0)
    assert products_computed() == []   # no GEMM ran: neither the root nor a derived placeholder


@pytest.mark.parametrize("use", ["probs", "shifted", "exp", "logsumexp_elsewhere", "broadcast_value",
                                 "keepdim_false", "first_dim"])
def test_other_spellings_materialise(use):
    def model():
        theta = sample_theta()
        eta = X @ theta
        if use == "probs":
            mi.sample("y", Categorical(probs=torch.softmax(eta, -1)))
        elif use == "shifted":
            mi.sample("y", Categorical(logits=eta + 1))
        elif use == "exp":
            mi.sample("y", Categorical(logits=eta.exp()))
        elif use == "logsumexp_elsewhere":
            mi.sample("z", Normal(eta.logsumexp(dim=-1, keepdim=True)[:, 0], 1.0))
            mi.sample("y", Categorical(logits=eta))
        elif use == "broadcast_value":
            mi.sample("y", Categorical(logits=eta.expand(2, N, C)))
        elif use == "keepdim_false":
            mi.sample("y", Categorical(logits=eta - eta.logsumexp(-1)[:, None]))
        else:
            mi.sample("y", Categorical(logits=eta - eta.logsumexp(0, keepdim=True)))

    y = Y.expand(2, N) if use == "broadcast_value" else Y
    t, theta = trace(mi.condition(model, y=y, z=torch.zeros(N)))
    site = next(s for s in t.sites if s.name == "y")
    real = torch.matmul(X, theta)   # [K, N, C]
    if use == "logsumexp_elsewhere":
        # the standalone logsumexp is its true value; the Categorical beside it stays native
        z = next(s for s in t.sites if s.name == "z")
        torch.testing.assert_close(z.tensors[0], real.logsumexp(-1))
        assert site.linear_X is X
        return
    assert site.linear_X is None
    assert products_computed() != []
    want = {"probs": Categorical(probs=torch.softmax(real, -1)).logits,
            "shifted": Categorical(logits=real + 1).logits,
            "exp": Categorical(logits=real.exp()).logits,
            "broadcast_value": Categorical(logits=real).logits[:, None].expand(K, 2, N, C),
            "keepdim_false": Categorical(logits=real).logits,
            "first_dim": Categorical(logits=real - real.logsumexp(1, keepdim=True)).logits}[use]
    torch.testing.assert_close(site.tensors[0], want)


def test_batched_value_materialises():
    def model():
        theta = sample_theta()
        y = mi.sample("y0", Bernoulli(torch.sigmoid(theta[0, 0])), sample_shape=N)
        mi.sample("y", Categorical(logits=X @ theta), )
        return y

    values = (torch.arange(K * N).reshape(K, N) % C)
    theta = torch.randn(K, P, C, generator=torch.Generator().manual_seed(0))
    t = particles.trace_particles(model, {"theta": theta, "y": values,
                                          "y0": torch.zeros(K, N)}, K)
    site = next(s for s in t.sites if s.name == "y")
    assert site.linear_X is None
    torch.testing.assert_close(site.tensors[0], Categorical(logits=torch.matmul(X, theta)).logits)


def test_vector_theta_recorded_as_before():
    def model():
        theta = mi.sample("theta", Normal(0.0, 1.0), sample_shape=P)
        mi.sample("y", Bernoulli(logits=X @ theta))

    theta = torch.randn(K, P, generator=torch.Generator().manual_seed(0))
    t = particles.trace_particles(mi.condition(model, y=(Y % 2).float()), {"theta": theta}, K)
    site = next(s for s in t.sites if s.name == "y")
    assert site.family == "bernoulli_logits" and site.linear_X is X
    assert site.linear_link == "identity" and site.linear_role == 0
    assert site.tensors[0].shape == (K, N) and site.tensors[0].stride() == (0, 0)
    torch.testing.assert_close(site.linear_theta, theta)
    assert products_computed() == []


def test_mv_of_a_matrix_theta_is_not_deferred():
    mode = DeferredMatmul(K)
    assert not mode._eligible((X, torch.zeros(P, C)), {}, matrix=False)


# ---- the C ABI on the CPU library ------------------------------------------------------------

def _site(**edits):
    X = torch.zeros(8, 3)
    theta = torch.zeros(2, 3, 4)
    y = torch.zeros(8, dtype=torch.int64)
    L = describe(X, theta, y, None, 1.0, 1.0)
    L._keep = (X, theta, y)
    for name, value in edits.items():
        setattr(L, name, value)
    return L


def test_struct_size_matches_the_mirror():
    size = ctypes.c_size_t()
    assert nat.lib().mi_softmax_linear_struct_size(ctypes.byref(size)) == 0
    assert size.value == ctypes.sizeof(nat.SoftmaxLinear)
    assert nat.lib().mi_softmax_linear_struct_size(None) == nat.MI_EINVAL


@pytest.mark.parametrize("edits", [
    {"K": 0}, {"N": 0}, {"P": 0}, {"C": 0}, {"P": 65}, {"C": nat.SOFTMAX_LINEAR_MAX_C + 1},
    {"x": None}, {"theta": None}, {"value": None}, {"value_kind": 7}],
    ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_invalid_arguments_are_rejected(edits):
    lib = nat.lib()
    L = _site(**edits)
    size = ctypes.c_size_t(12345)
    assert lib.mi_softmax_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == nat.MI_EINVAL
    out = torch.zeros(64)
    flags = torch.zeros(1, dtype=torch.int32)
    work = torch.zeros(1 << 16, dtype=torch.uint8)
    assert lib.mi_softmax_linear_forward(ctypes.byref(L), work.data_ptr(), work.numel(),
                                         out.data_ptr(), None, flags.data_ptr(), None) == nat.MI_EINVAL


def test_null_outputs_and_small_workspace_are_rejected():
    lib = nat.lib()
    L = _site()
    size = ctypes.c_size_t()
    assert lib.mi_softmax_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == 0
    assert size.value >= 2 * 3 * 4 * 4 + 2 * 8
    assert lib.mi_softmax_linear_workspace_bytes(ctypes.byref(L), None) == nat.MI_EINVAL
    assert lib.mi_softmax_linear_workspace_bytes(None, ctypes.byref(size)) == nat.MI_EINVAL
    out = torch.zeros(64)
    flags = torch.zeros(1, dtype=torch.int32)
    work = torch.zeros(size.value, dtype=torch.uint8)
    args = (out.data_ptr(), None, flags.data_ptr(), None)
    assert lib.mi_softmax_linear_forward(None, work.data_ptr(), size.value, *args) == nat.MI_EINVAL
    assert lib.mi_softmax_linear_forward(ctypes.byref(L), work.data_ptr(), size.value, None, None,
                                         flags.data_ptr(), None) == nat.MI_EINVAL
    assert lib.mi_softmax_linear_forward(ctypes.byref(L), work.data_ptr(), size.value,
                                         out.data_ptr(), None, None, None) == nat.MI_EINVAL
    assert lib.mi_softmax_linear_forward(ctypes.byref(L), None, size.value, *args) == nat.MI_EWORKSPACE
    assert lib.mi_softmax_linear_forward(ctypes.byref(L), work.data_ptr(), size.value - 1,
                                         *args) == nat.MI_EWORKSPACE


# ---- the references ---------------------------------------------------------------------------

def test_fp64_reference_matches_torch():
    rng = np.random.default_rng(3)
    Xn = rng.standard_normal((40, 5))
    th = rng.standard_normal((3, 5, 6))
    y = rng.integers(0, 6, 40)
    mask = rng.random(40) < 0.7
    total, dtheta, _, _ = reference(Xn, th, y.astype(np.float64), mask, 2.5, -0.5)
    tt = torch.tensor(th, requires_grad=True)
    lp = Categorical(logits=torch.tensor(Xn) @ tt).log_prob(torch.tensor(y))
    want = 2.5 * (lp * torch.tensor(mask)).sum(-1)
    (-0.5 * want.sum()).backward()
    np.testing.assert_allclose(total, want.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dtheta, tt.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", gpu.CASES, ids=lambda c: c.id)
def test_float32_restatement_meets_the_bounds(case):
    Xn, theta, y, mask, row_index = gpu.inputs(case)
    total, dtheta = float32_restatement(Xn, theta, y.astype(np.float64), mask, gpu.SITE_SCALE, gpu.G0,
                                        row_index)
    ft, fd = gpu.fractions(total, dtheta, case)
    print(f"\n{case.id}: restatement at {ft:.3f} of the total's bound, {fd:.3f} of dtheta's")
    assert ft <= 1.0 and fd <= 1.0, (ft, fd)
