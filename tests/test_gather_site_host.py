"""
Group-indexed sites on the host: the trace records the native spellings of ``alpha[group]`` as
gathered sites without computing the gather, every other spelling materialises exactly torch's
values, the index plan, the invalid-argument returns of mi_gather_site_forward (before any device
work), the fp64 reference of tests/gather_site_reference.py against torch.distributions and
autograd through a real gather, and the float32 restatement of the kernel against the GPU file's
bounds on every one of its input sets.
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Normal, Poisson

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd import particles
from mininf_amd.engine.gather import index_plan
from mininf_amd.linear import DeferredMatmul
from tests import test_gpu_gather_site as gpu
from tests.gather_site_reference import (describe, float32_restatement, reference, sort_plan,
                                         tensors_of)

K, G, N = 3, 4, 9


@pytest.fixture(autouse=True)
def host_deferral(monkeypatch):
    monkeypatch.setattr(DeferredMatmul, "require_device", False)


class Spy(torch.overrides.TorchFunctionMode):
    """Counts the gathers that run on a batched tensor."""
    NAMES = ("__getitem__", "index_select", "gather", "index_put", "index_put_", "take")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in self.NAMES and args and \
                isinstance(args[0], torch.Tensor) and torch._C._functorch.is_batchedtensor(args[0]):
            self.seen.append(func.__name__)
        return func(*args, **(kwargs or {}))


def _trace(build, data=None, states=None):
    torch.manual_seed(0)
    group = torch.tensor([3, 0, 1, 1, 3, 0, 0, 1, 3])
    y = torch.randn(N) if data is None else data
    states = states or {"alpha": torch.randn(K, G), "sigma": torch.rand(K) + 0.5,
                        "a": torch.randn(K), "b": torch.randn(K)}

    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        sigma = mi.sample("sigma", Normal(0, 1))
        a = mi.sample("a", Normal(0, 1))
        b = mi.sample("b", Normal(0, 1))
        mi.sample("y", build(alpha, group, sigma, a, b))
    spy = Spy()
    with spy:
        trace = particles.trace_particles(mi.condition(model, y=y), states, K)
    site = next(s for s in trace.sites if s.name == "y")
    return site, states, group, spy.seen


SPELLINGS = {
    "getitem": lambda al, g, s, a, b: Normal(al[g], s),
    "index_select": lambda al, g, s, a, b: Normal(torch.index_select(al, 0, g), s),
    "method_index_select": lambda al, g, s, a, b: Normal(al.index_select(0, g), 1.5),
    "keyword_index_select": lambda al, g, s, a, b: Normal(al.index_select(dim=0, index=g), s),
    "expand": lambda al, g, s, a, b: Normal(al[g].expand(N), s),
    "negative": lambda al, g, s, a, b: Normal(al[g - G], s),
    "int32": lambda al, g, s, a, b: Normal(al[g.int()], s),
    "scale": lambda al, g, s, a, b: Normal(a, al[g], validate_args=False),
    "bernoulli": lambda al, g, s, a, b: Bernoulli(logits=al[g]),
    "poisson": lambda al, g, s, a, b: Poisson(al[g].exp()),
    "poisson_torch_exp": lambda al, g, s, a, b: Poisson(torch.exp(al[g])),
    "add": lambda al, g, s, a, b: Normal(al[g] + a, s),
    "radd": lambda al, g, s, a, b: Normal(a + al[g], s),
    "number_radd": lambda al, g, s, a, b: Normal(2.0 + al[g], s),
    "sub": lambda al, g, s, a, b: Normal(al[g] - a, s),
    "rsub": lambda al, g, s, a, b: Normal(1.0 - al[g], s),
    "tensor_rsub": lambda al, g, s, a, b: Normal(a - al[g], s),
    "mul": lambda al, g, s, a, b: Normal(al[g] * b, s),
    "rmul": lambda al, g, s, a, b: Normal(0.5 * al[g], s),
    "affine": lambda al, g, s, a, b: Normal(a + b * al[g], s),
    "torch_affine": lambda al, g, s, a, b: Normal(torch.add(torch.mul(al[g], b), a), s),
    "poisson_affine": lambda al, g, s, a, b: Poisson((a + b * al[g]).exp()),
    "chain": lambda al, g, s, a, b: Normal((al[g] + 1.0) * b - a, s),
}


def _data(spelling):
    torch.manual_seed(1)
    if "poisson" in spelling:
        return torch.poisson(torch.ones(N) * 2)
    if spelling == "bernoulli":
        return (torch.rand(N) < 0.5).float()
    return torch.randn(N)


@pytest.mark.parametrize("spelling", list(SPELLINGS))
def test_native_spellings_are_recorded_without_a_gather(spelling):
    site, states, group, seen = _trace(SPELLINGS[spelling], _data(spelling))
    assert seen == [], seen
    roles = [g for g in site.gather_roles if g is not None]
    assert len(roles) == 1
    role = roles[0]
    assert role.table.data_ptr() == states["alpha"].data_ptr() and role.table.shape == (K, G)
    assert role.link == ("exp" if "poisson" in spelling else "identity")
    # the predictor the record stands for is the one the model wrote
    al, s, a, b = states["alpha"], states["sigma"], states["a"], states["b"]
    index = role.index.long()
    gathered = al[:, index]
    eta = gathered
    if role.mult is not None:
        eta = (role.mult.reshape(K, 1) if isinstance(role.mult, torch.Tensor) else role.mult) * eta
    if role.shift is not None:
        eta = (role.shift.reshape(K, 1) if isinstance(role.shift, torch.Tensor)
               else role.shift) + eta
    want = torch.stack([getattr(SPELLINGS[spelling](al[k], group, s[k], a[k], b[k]),
                                {"scale": "scale", "bernoulli": "logits"}.get(
                                    spelling, "rate" if "poisson" in spelling else "loc"))
                        for k in range(K)])
    got = eta.exp() if role.link == "exp" else eta
    torch.testing.assert_close(got, want.expand(K, N), rtol=1e-6, atol=1e-6)
    if spelling in ("getitem", "affine", "add"):   # the scale beside it stays one scalar per particle
        assert site.tensors[1].shape == (K,)


OTHERS = {
    "power": lambda al, g, s, a, b: Normal(al[g] ** 2, s),
    "index_2d": lambda al, g, s, a, b: Normal(al[g.reshape(3, 3)].reshape(N), s),
    "slice": lambda al, g, s, a, b: Normal(torch.cat([al[1:], al[:2], al]), s),
    "boolean": lambda al, g, s, a, b: Normal(torch.cat([al[g[:4] > 0], al[g[:4] < 9], al[:2]])[:N], s),
    "exp_then_add": lambda al, g, s, a, b: Normal(al[g].exp() + a, s),
    "probs": lambda al, g, s, a, b: Bernoulli(probs=torch.sigmoid(al[g])),
    "two_indices": lambda al, g, s, a, b: Normal(al[g], al[g.flip(0)].exp()),
    "normal_exp_loc": lambda al, g, s, a, b: Normal(al[g].exp(), s),
    "poisson_identity": lambda al, g, s, a, b: Poisson(al[g] * al[g] + 1.0),
}


@pytest.mark.parametrize("spelling", list(OTHERS))
def test_everything_else_materialises_torchs_values(spelling):
    data = (torch.rand(N) < 0.5).float() if spelling == "probs" else \
        torch.poisson(torch.ones(N)) if "poisson" in spelling else None
    site, states, group, _ = _trace(OTHERS[spelling], data)
    assert site.gather_roles is None
    al, s, a, b = states["alpha"], states["sigma"], states["a"], states["b"]
    for role, name in enumerate(("probs",) if spelling == "probs" else
                                ("rate",) if "poisson" in spelling else ("loc", "scale")):
        want = torch.stack([torch.as_tensor(getattr(OTHERS[spelling](al[k], group, s[k], a[k], b[k]),
                                                    name)).expand(N) for k in range(K)])
        assert torch.equal(site.tensors[role].expand(K, N), want), name


def test_batched_index_and_batched_value_materialise():
    site, states, group, _ = _trace(
        lambda al, g, s, a, b: Normal(al[(g + (a > 0).long()) % G], s))
    assert site.gather_roles is None
    states = {"alpha": torch.randn(K, G), "sigma": torch.rand(K) + 0.5, "a": torch.randn(K),
              "b": torch.randn(K), "y": torch.randn(K, N)}
    group = torch.arange(N) % G

    def model():
        alpha = mi.sample("alpha", Normal(0, 1), sample_shape=(G,))
        sigma = mi.sample("sigma", Normal(0, 1))
        mi.sample("a", Normal(0, 1))
        mi.sample("b", Normal(0, 1))
        mi.sample("y", Normal(alpha[group], sigma), sample_shape=())
    trace = particles.trace_particles(model, states, K)
    site = next(s for s in trace.sites if s.name == "y")
    assert site.gather_roles is None
    assert torch.equal(site.tensors[0], states["alpha"][:, group])


@pytest.mark.parametrize("spelling", ["getitem", "affine", "chain", "tensor_rsub", "rmul",
                                      "poisson_affine", "torch_affine"])
def test_declined_plan_puts_back_exactly_what_the_model_wrote(spelling):
    from mininf_amd.engine.gather import _materialise
    site, states, group, _ = _trace(SPELLINGS[spelling], _data(spelling))
    _materialise(site, K)
    assert site.gather_roles is None
    al, s, a, b = states["alpha"], states["sigma"], states["a"], states["b"]
    name = "rate" if "poisson" in spelling else "loc"
    want = torch.stack([getattr(SPELLINGS[spelling](al[k], group, s[k], a[k], b[k]), name)
                        for k in range(K)])
    assert torch.equal(site.tensors[0], want)


def test_switch_turns_the_deferral_off(monkeypatch):
    monkeypatch.setenv("MININF_AMD_DEFER_GATHER", "0")
    site, states, group, seen = _trace(SPELLINGS["getitem"])
    assert site.gather_roles is None and seen == ["__getitem__"]
    assert torch.equal(site.tensors[0], states["alpha"][:, group])


def test_index_plan():
    index = torch.tensor([2, -1, 0, 2, -3, 0, 3, 2])   # G = 4: wraps to 2 3 0 2 1 0 3 2
    order, sg = index_plan(index, 4)
    assert order.dtype == sg.dtype == torch.int32
    assert sg.tolist() == [0, 0, 1, 2, 2, 2, 3, 3]
    assert order.tolist() == [2, 5, 4, 0, 3, 7, 1, 6]   # stable: rows of a group in their order
    assert index_plan(index, 4)[0] is order             # memoised
    index[0] = 1
    assert index_plan(index, 4)[1].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]   # a new version: replanned
    assert index_plan(torch.tensor([0, 4]), 4) is None and index_plan(torch.tensor([-5]), 4) is None
    ref_order, ref_sg = sort_plan(index.numpy(), 4)
    assert np.array_equal(ref_order, index_plan(index, 4)[0].numpy())
    assert np.array_equal(ref_sg, index_plan(index, 4)[1].numpy())


def _site(**changes):
    case = gpu.make_case(0, "normal", ["g", "p"], 3, 10, 4, np.arange(10) % 4,
                         shift="pointer", mult="pointer")
    tensors = tensors_of(case, "cpu")
    order, sg = (torch.from_numpy(x) for x in sort_plan(case["index"], 4))
    L = describe(case, tensors, order, sg)
    keep = (tensors, order, sg)
    for name, value in changes.items():
        target = L
        *path, leaf = name.split(".")
        for part in path:
            target = target.role[int(part[-1])]
        setattr(target, leaf, value)
    return L, keep


def test_struct_size():
    size = ctypes.c_size_t()
    assert nat.lib().mi_gather_site_struct_size(ctypes.byref(size)) == 0
    assert size.value == ctypes.sizeof(nat.GatherSite)
    assert nat.lib().mi_gather_site_struct_size(None) == nat.MI_EINVAL


@pytest.mark.parametrize("changes", [
    {"K": 0}, {"N": 0}, {"G": 0}, {"family": 3}, {"family": -1}, {"order": None},
    {"sorted_group": None}, {"value": None}, {"value_kind": 2},
    {"role0.kind": 4}, {"role0.kind": nat.GATHER_PARTICLE}, {"role0.data": None},
    {"role1.data": None}, {"role0.link": 2}, {"role0.shift_kind": 3}, {"role0.mult_kind": -1},
    {"role0.shift": None}, {"role0.mult": None}])
def test_invalid_arguments_return_before_any_device_work(changes):
    L, keep = _site(**changes)
    lib = nat.lib()
    size = ctypes.c_size_t()
    assert lib.mi_gather_site_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == nat.MI_EINVAL
    work = torch.zeros(1 << 16, dtype=torch.uint8)
    total, flags = torch.zeros(3), torch.zeros(1, dtype=torch.int32)
    assert lib.mi_gather_site_forward(ctypes.byref(L), work.data_ptr(), work.numel(),
                                      total.data_ptr(), None, flags.data_ptr(), None) == nat.MI_EINVAL


def test_null_outputs_and_small_workspace():
    L, keep = _site()
    lib = nat.lib()
    size = ctypes.c_size_t()
    assert lib.mi_gather_site_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == 0
    assert size.value > 0
    assert lib.mi_gather_site_workspace_bytes(ctypes.byref(L), None) == nat.MI_EINVAL
    assert lib.mi_gather_site_workspace_bytes(None, ctypes.byref(size)) == nat.MI_EINVAL
    work = torch.zeros(size.value, dtype=torch.uint8)
    total, flags = torch.zeros(3), torch.zeros(1, dtype=torch.int32)
    fwd = lib.mi_gather_site_forward
    assert fwd(None, work.data_ptr(), size.value, total.data_ptr(), None, flags.data_ptr(),
               None) == nat.MI_EINVAL
    assert fwd(ctypes.byref(L), work.data_ptr(), size.value, None, None, flags.data_ptr(),
               None) == nat.MI_EINVAL
    assert fwd(ctypes.byref(L), work.data_ptr(), size.value, total.data_ptr(), None, None,
               None) == nat.MI_EINVAL
    assert fwd(ctypes.byref(L), None, size.value, total.data_ptr(), None, flags.data_ptr(),
               None) == nat.MI_EWORKSPACE
    assert fwd(ctypes.byref(L), work.data_ptr(), size.value - 1, total.data_ptr(), None,
               flags.data_ptr(), None) == nat.MI_EWORKSPACE


def _torch_reference(case):
    """The case through torch.distributions and autograd through a real gather, in fp64."""
    K_, N_, G_ = case["K"], case["N"], case["G"]
    index = torch.from_numpy(np.where(case["index"] < 0, case["index"] + G_, case["index"]))
    leaves, a = {}, []

    def leaf(name, array):
        leaves[name] = torch.tensor(np.asarray(array, np.float64), requires_grad=True)
        return leaves[name]
    for r, role in enumerate(case["roles"]):
        if role[0] == "gather":
            eta = leaf(f"role{r}", role[1])[:, index]
            if role[3] is not None:
                eta = (leaf(f"mult{r}", role[3]).reshape(K_, 1) if isinstance(role[3], np.ndarray)
                       else role[3]) * eta
            if role[2] is not None:
                eta = (leaf(f"shift{r}", role[2]).reshape(K_, 1) if isinstance(role[2], np.ndarray)
                       else role[2]) + eta
            a.append(eta.exp() if role[4] == "exp" else eta)
        elif role[0] == "particle":
            a.append(leaf(f"role{r}", role[1]).reshape(K_, 1).expand(K_, N_))
        elif role[0] == "data":
            a.append(torch.tensor(np.asarray(role[1], np.float64)).expand(K_, N_))
        else:
            a.append(torch.full((K_, N_), float(role[1]), dtype=torch.float64))
    value = torch.tensor(np.asarray(case["value"], np.float64))
    dist = {"normal": lambda: Normal(a[0], a[1]), "bernoulli": lambda: Bernoulli(logits=a[0]),
            "poisson": lambda: Poisson(a[0])}[case["family"]]()
    lp = dist.log_prob(value.expand(K_, N_))
    if case["mask"] is not None:
        lp = torch.where(torch.from_numpy(case["mask"]), lp, torch.zeros_like(lp))
    total = case["site_scale"] * lp.sum(1)
    (total.sum() * case["g0"]).backward()
    return total.detach().numpy(), {name: t.grad.numpy() for name, t in leaves.items()
                                    if t.grad is not None}


@pytest.mark.parametrize("name", list(gpu.CASES)[::3])
def test_reference_agrees_with_torch(name):
    case = gpu.CASES[name]
    ref = reference(case)
    total, grads = _torch_reference(case)
    np.testing.assert_allclose(ref["total"][0], total, rtol=1e-10, atol=1e-10)
    for key, (value, _) in ref.items():
        if key != "total":
            np.testing.assert_allclose(value, grads[key], rtol=1e-9, atol=1e-11, err_msg=key)


@pytest.mark.parametrize("name", list(gpu.CASES))
def test_float32_restatement_meets_the_gpu_bounds(name):
    case = gpu.CASES[name]
    worst = gpu.check(case, float32_restatement(case), "restatement")
    print(name, worst)
