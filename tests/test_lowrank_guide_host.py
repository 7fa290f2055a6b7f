"""
The native LowRankMultivariateNormal guide factor, as far as a CPU-only host can see it: the
library exports the sampler's three functions with ctypes signatures, their argument checks run
before any device work, and a factor the native path does not take (host-resident, batched,
float64, rank beyond the cap, a subclass) keeps torch's own rsample and entropy.
"""
import ctypes

import torch
from torch.distributions import LowRankMultivariateNormal

from mininf_amd import _native as nat, engine, guide
from mininf_amd.nn import ParameterizedDistribution

SYMBOLS = ("mi_lowrank_rsample", "mi_lowrank_rsample_backward_workspace_bytes",
           "mi_lowrank_rsample_backward")


def test_library_exports_lowrank_sampler():
    lib = nat.lib()
    for name in SYMBOLS:
        assert name in nat._SIGNATURES, name
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == list(nat._SIGNATURES[name][1])
    assert len(nat._SIGNATURES["mi_lowrank_rsample"][1]) == 14
    assert len(nat._SIGNATURES["mi_lowrank_rsample_backward"][1]) == 19
    assert nat.LOWRANK_MAX_R == 128 and nat.LOWRANK_MAX_D == 1 << 24


def test_argument_checks_run_before_any_device_work():
    """Null pointers throughout: a check that came after any device work would fault."""
    lib = nat.lib()
    size = ctypes.c_size_t(0)

    def forward(K, D, R):
        return lib.mi_lowrank_rsample(None, None, None, K, D, R, 0, 0, None, 0, 0, None, None, None)

    def backward(K, D, R):
        return lib.mi_lowrank_rsample_backward(None, 1, 1, None, K, D, R, 0, 0, None, 0, 0, None,
                                               None, 0, None, None, None, None)

    def workspace(K, D, R):
        return lib.mi_lowrank_rsample_backward_workspace_bytes(K, D, R, ctypes.byref(size))

    for call in (forward, backward, workspace):
        assert call(0, 1, 1) == nat.MI_EINVAL
        assert call(1, 0, 1) == nat.MI_EINVAL
        assert call(1, 1, 0) == nat.MI_EINVAL
        assert call(-3, 2, 1) == nat.MI_EINVAL
        assert call(1, 2, nat.LOWRANK_MAX_R + 1) == nat.MI_EUNSUPPORTED
        assert call(1, nat.LOWRANK_MAX_D + 1, 1) == nat.MI_EUNSUPPORTED
    # in range, but no arrays: refused, still before any device work
    assert forward(1, 2, 1) == nat.MI_EINVAL
    assert backward(1, 2, 1) == nat.MI_EINVAL
    assert lib.mi_lowrank_rsample_backward_workspace_bytes(1, 1, 1, None) == nat.MI_EINVAL
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.mi_lowrank_rsample(p, p, p, 1, 2, 1, 0, 0, None, 1 << 24, 0, None, p,
                                  None) == nat.MI_EINVAL
    # one particle slice needs no workspace; several need [slices, D * R + 2 D] floats
    assert workspace(32, 1 << 20, 64) == 0 and size.value == 0
    assert workspace(256, 64, 64) == 0
    assert size.value > 0 and size.value % (4 * (64 * 64 + 2 * 64)) == 0
    assert workspace(4096, 3, 2) == 0
    assert size.value > 0 and size.value % (4 * (3 * 2 + 2 * 3)) == 0
    # a backward that needs a workspace and gets none is refused before it launches
    assert lib.mi_lowrank_rsample_backward(p, 1, 1, p, 256, 64, 64, 0, 0, None, 0, 0, None, None,
                                           0, p, p, p, None) == nat.MI_EWORKSPACE


class _Subclass(LowRankMultivariateNormal):
    pass


def _factors():
    D, R = 5, 2
    host = LowRankMultivariateNormal(torch.zeros(D), 0.1 * torch.ones(D, R), torch.ones(D))
    batched = LowRankMultivariateNormal(torch.zeros(2, D), 0.1 * torch.ones(D, R), torch.ones(D))
    double = LowRankMultivariateNormal(torch.zeros(D, dtype=torch.float64),
                                       0.1 * torch.ones(D, R, dtype=torch.float64),
                                       torch.ones(D, dtype=torch.float64))
    wide = LowRankMultivariateNormal(torch.zeros(D), 0.01 * torch.ones(D, nat.LOWRANK_MAX_R + 1),
                                     torch.ones(D))
    sub = _Subclass(torch.zeros(D), 0.1 * torch.ones(D, R), torch.ones(D))
    return {"host": host, "batched": batched, "double": double, "wide": wide, "sub": sub}


def test_other_lowrank_factors_keep_the_torch_path():
    K = 6
    factors = _factors()
    for name, factor in factors.items():
        assert not guide.native_lowrank(factor), name
    assert not guide.native_lowrank(torch.distributions.Normal(0.0, 1.0))
    fused, rest = engine.entropy_factors(factors)
    assert fused == [] and rest == list(factors.values())
    # the draws come from torch's rsample, on the host, through the unchanged fallback
    torch.manual_seed(3)
    samples = guide.draw_all(factors, K, seed=1, step=0, particle_offset=0)
    torch.manual_seed(3)
    want = {name: factor.rsample(torch.Size([K])) for name, factor in factors.items()}
    assert guide.counts()["lowrank_draws"] == 0
    for name in want:
        assert samples[name].device.type == "cpu"
        assert torch.equal(samples[name], want[name])
    assert samples["host"].shape == (K, 5) and samples["batched"].shape == (K, 2, 5)


def test_host_lowrank_guide_evaluates_through_torch():
    """A host-resident low-rank guide: draws, entropy and their gradients are torch's own."""
    D, R, K = 4, 2, 6
    module = ParameterizedDistribution(LowRankMultivariateNormal, loc=torch.zeros(D),
                                       cov_factor=0.1 * torch.ones(D, R),
                                       cov_diag=0.5 * torch.ones(D))
    factor = module()
    assert type(factor) is LowRankMultivariateNormal
    assert not guide.native_lowrank(factor)
    fused, rest = engine.entropy_factors({"theta": factor})
    assert fused == [] and rest == [factor]
    samples = guide.draw_all({"theta": factor}, K, seed=1, step=0, particle_offset=0)
    z = samples["theta"]
    assert guide.counts()["lowrank_draws"] == 0
    assert z.shape == (K, D) and z.grad_fn is not None
    value = z.square().sum() / K - sum(f.entropy().sum() for f in rest)
    value.backward()
    for p in module.distribution_parameters.values():
        assert p.grad is not None and torch.isfinite(p.grad).all()


def test_a_data_sharded_lowrank_factor_is_refused():
    factor = _factors()["host"]
    cfg = guide.DrawConfig(K=2, seed=1, step=0, stream_id=0, particle_offset=0, sharded=True)
    try:
        guide.draw(factor, cfg)
    except nat.NativeError as error:
        assert "must be a Normal" in str(error)
    else:
        raise AssertionError("a data-sharded low-rank factor was drawn")
