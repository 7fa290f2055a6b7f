"""
mi_gather_slopes on the host: the struct mirror, the invalid-argument returns of both entry points
(before any device work), the fp64 reference of tests/gather_slopes_reference.py against
torch.distributions and autograd through real gathers and real products, and the float32
restatement of the kernel -- the same fmaf order, the same batch folds -- against the GPU file's
bounds on every one of its input sets: the inputs leave the bounds attainable.
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Normal, Poisson

from mininf_amd import _native as nat
from tests import test_gpu_gather_slopes_site as gpu
from tests.gather_slopes_reference import Z_LAYOUTS, float32_restatement, reference


def test_struct_size():
    size = ctypes.c_size_t()
    assert nat.lib().mi_gather_slopes_struct_size(ctypes.byref(size)) == 0
    assert size.value == ctypes.sizeof(nat.GatherSlopes)
    assert nat.lib().mi_gather_slopes_struct_size(None) == nat.MI_EINVAL
    assert nat.GatherSlopes.linear.offset == 0 and nat.GatherSlopes.S.offset == \
        ctypes.sizeof(nat.GatherLinear)
    assert ctypes.sizeof(nat.GatherSlopes) == ctypes.sizeof(nat.GatherLinear) + 8 + \
        nat.GATHER_MAX_SLOPES * ctypes.sizeof(nat.GatherSlope)


def test_invalid_arguments_return_before_any_device_work():
    gpu.argument_errors("cpu")


def test_shapes_cover_every_pair():
    shapes = gpu._shapes()   # (asserts the cover itself)
    assert {s[3] for s in shapes} == set(gpu.SS) and {s[4] for s in shapes} == set(gpu.PS)
    assert len(shapes) <= 60
    cases = gpu.CASES.values()
    assert {case["z_layout"] for case in cases} == set(Z_LAYOUTS)
    for family in ("normal", "bernoulli", "poisson"):
        assert any(case["family"] == family for case in cases)
    assert {case["roles"][1][0] for case in cases if len(case["roles"]) > 1} == \
        {"particle", "constant", "data", "gather"}
    assert any(case.get("null_slopes") for case in cases)
    assert any(any(n.startswith("slope") for n in case["null"]) for case in cases)
    assert any(case["strided"] for case in cases)
    assert {None if case["mask"] is None else bool(case["mask"].any()) for case in cases} == \
        {None, True, False}


def _torch_reference(case):
    """The case through torch.distributions and autograd through real gathers, in fp64."""
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
            if r == 0:
                for s, (beta, z) in enumerate(case["slopes"]):
                    eta = eta + leaf(f"slope{s}", beta)[:, index] * torch.tensor(
                        np.asarray(z, np.float64))
                eta = eta + leaf("dtheta", case["theta"]) @ torch.tensor(
                    np.asarray(case["X"], np.float64)).t()
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
    assert "dtheta" in ref and "slope0" in ref
    for key, (value, _) in ref.items():
        if key != "total":
            np.testing.assert_allclose(value, grads[key], rtol=1e-9, atol=1e-11, err_msg=key)


@pytest.mark.parametrize("name", list(gpu.CASES))
def test_float32_restatement_meets_the_gpu_bounds(name):
    case = gpu.CASES[name]
    got = float32_restatement(case)
    assert set(got) == {"total", *gpu._names(case)}
    worst = gpu.check(case, got, "restatement")
    print(name, worst)
