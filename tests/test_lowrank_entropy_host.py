"""
The native LowRankMultivariateNormal entropy, as far as a CPU-only host can see it: the library
exports mi_lowrank_entropy and its workspace query, their argument checks run before any device
work, the closed form the GPU tests compare against (tests/lowrank_entropy_reference.py) is
float64 autograd of torch's own entropy(), and a factor the native path does not take keeps
torch's entropy.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.distributions import LowRankMultivariateNormal

from mininf_amd import _native as nat, guide, nn
from tests import lowrank_entropy_reference as ref

SYMBOLS = ("mi_lowrank_entropy_workspace_bytes", "mi_lowrank_entropy")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "mininf_amd.h")


def test_library_exports_lowrank_entropy():
    with open(HEADER) as fh:
        header = fh.read()
    lib = nat.lib()
    for name in SYMBOLS:
        assert f"int {name}(" in header, name
        assert name in nat.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == list(nat._SIGNATURES[name][1])
    assert len(nat._SIGNATURES["mi_lowrank_entropy_workspace_bytes"][1]) == 3
    assert len(nat._SIGNATURES["mi_lowrank_entropy"][1]) == 11


def test_argument_checks_run_before_any_device_work():
    """Pointers that no device could read: a check that came after any device work would fault."""
    lib = nat.lib()
    size = ctypes.c_size_t(0)
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)

    def entropy(D, R, W=p, d=p, L=p, ws=p, ws_bytes=1 << 40, out=p, dW=None, dd=None):
        return lib.mi_lowrank_entropy(W, d, L, D, R, ws, ws_bytes, out, dW, dd, None)

    def workspace(D, R):
        return lib.mi_lowrank_entropy_workspace_bytes(D, R, ctypes.byref(size))

    for call in (entropy, workspace):
        assert call(2, nat.LOWRANK_MAX_R + 1) == nat.MI_EUNSUPPORTED
        assert call(nat.LOWRANK_MAX_D + 1, 1) == nat.MI_EUNSUPPORTED
        assert call(0, 1) == nat.MI_EINVAL
        assert call(1, 0) == nat.MI_EINVAL
    assert nat.MI_EINVAL == -1
    assert lib.mi_lowrank_entropy_workspace_bytes(3, 2, None) == nat.MI_EINVAL
    assert entropy(3, 2, W=None) == nat.MI_EINVAL
    assert entropy(3, 2, d=None) == nat.MI_EINVAL
    assert entropy(3, 2, L=None) == nat.MI_EINVAL
    assert entropy(3, 2, out=None) == nat.MI_EINVAL
    assert entropy(3, 2, dW=p) == nat.MI_EINVAL   # one gradient without the other
    assert entropy(3, 2, dd=p) == nat.MI_EINVAL
    # C^-1, the log-determinant word and one partial per block of the row pass, at the least
    for D, R in ((3, 2), (4100, 64), (1 << 24, 128)):
        assert workspace(D, R) == 0
        assert size.value >= 4 * R * R + 8 + 8
        assert entropy(D, R, ws_bytes=size.value - 1) == nat.MI_EINVAL
        assert entropy(D, R, ws=None, ws_bytes=size.value) == nat.MI_EINVAL


@pytest.mark.parametrize("D,R", ((1, 1), (3, 2), (33, 33), (130, 128)))
def test_closed_form_is_float64_autograd_of_torch_entropy(D, R):
    """Guards the yardstick, not the feature: 1e-12 absolute is the order of float64 rounding here
    (largest difference observed: 8e-16)."""
    W, d, L = ref.inputs(D, R, ref.case_seed(D, R))
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    dt = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    factor = LowRankMultivariateNormal(torch.zeros(D, dtype=torch.float64), Wt, dt)
    H = factor.entropy()
    H.backward()
    # the float64 factor of the same W and d, not its float32 rounding
    got_H, got_W, got_d, _ = ref.closed_form(W, d, factor._capacitance_tril.detach().numpy())
    errors = (abs(got_H - float(H.detach())), np.abs(got_W - Wt.grad.numpy()).max(),
              np.abs(got_d - dt.grad.numpy()).max())
    print(f"D={D} R={R}: |dH| {errors[0]:.3g} |ddW| {errors[1]:.3g} |ddd| {errors[2]:.3g}")
    assert max(errors) <= 1e-12, errors


def test_input_maker_is_well_conditioned():
    for D, R in ((33, 33), (130, 128), (4100, 64)):
        W, d, L = ref.inputs(D, R, ref.case_seed(D, R))
        assert W.dtype == np.float64 and (W == W.astype(np.float32)).all()
        assert (L == L.astype(np.float32)).all() and (np.triu(L, 1) == 0).all()
        assert 0.5 <= d.min() and d.max() <= 2.0
        assert np.linalg.cond(np.eye(R) + W.T @ (W / d[:, None])) < 60


class _Subclass(LowRankMultivariateNormal):
    pass


def test_other_lowrank_factors_keep_the_torch_entropy():
    D, R = 5, 2
    factors = {
        "host": LowRankMultivariateNormal(torch.zeros(D), 0.1 * torch.ones(D, R), torch.ones(D)),
        "batched": LowRankMultivariateNormal(torch.zeros(2, D), 0.1 * torch.ones(D, R),
                                             torch.ones(D)),
        "double": LowRankMultivariateNormal(torch.zeros(D, dtype=torch.float64),
                                            0.1 * torch.ones(D, R, dtype=torch.float64),
                                            torch.ones(D, dtype=torch.float64)),
        "wide": LowRankMultivariateNormal(torch.zeros(D),
                                          0.01 * torch.ones(D, nat.LOWRANK_MAX_R + 1),
                                          torch.ones(D)),
        "sub": _Subclass(torch.zeros(D), 0.1 * torch.ones(D, R), torch.ones(D)),
    }
    guide.draw_all(factors, 4, seed=1, step=0, particle_offset=0)
    for name, factor in factors.items():
        assert not guide.native_lowrank(factor), name
        # the term the loss subtracts for a factor of the rest
        assert torch.equal(guide.entropy(factor), factor.entropy().sum()), name
    assert guide.counts()["lowrank_entropies"] == 0


def test_host_lowrank_guide_entropy_gradient_is_torchs():
    """A host-resident guide: the entropy term reaches the parameters through torch's graph."""
    D, R = 4, 2
    module = nn.ParameterizedDistribution(LowRankMultivariateNormal, loc=torch.zeros(D),
                                          cov_factor=0.1 * torch.ones(D, R),
                                          cov_diag=0.5 * torch.ones(D))
    factor = module()
    guide.draw_all({"theta": factor}, 4, seed=1, step=0, particle_offset=0)
    guide.entropy(factor).backward()
    assert guide.counts()["lowrank_entropies"] == 0
    params = module.distribution_parameters
    assert params["loc"].grad is None or not params["loc"].grad.any()
    for name in ("cov_factor", "cov_diag"):
        assert torch.isfinite(params[name].grad).all() and params[name].grad.any()
