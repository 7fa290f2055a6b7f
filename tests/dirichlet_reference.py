"""
Float64 CPU references for the Dirichlet kernels (tests/test_gpu_dirichlet.py), written from the
formulas rather than through ``torch.distributions.Dirichlet``; tests/test_dirichlet_host.py checks
them against torch's own ``log_prob`` / ``entropy`` / ``rsample`` backward. Inputs are the float32
tensors the kernels read, promoted to float64.
"""
import torch
from torch.distributions.dirichlet import _Dirichlet_backward

FLT_MIN = 1.17549435e-38
ONE_BELOW = 1.0 - 2.0 ** -24


def log_prob(concentration: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    """dirichlet.py:93-97 in float64 (differentiable in both arguments)."""
    a, x = concentration.double(), value.double()
    return torch.xlogy(a - 1.0, x).sum(-1) + torch.lgamma(a.sum(-1)) - torch.lgamma(a).sum(-1)


def density(concentration, value, mask=None, scale=1.0, g0=1.0):
    """
    What ``mi_dirichlet_forward`` returns for concentration / value [K, N, C] (float32, broadcast
    views allowed): total [K] and the dense gradients g0 * d total / d (concentration, value) per
    [K, N, C] entry, all float64.
    """
    a = concentration.detach().double().clone().requires_grad_()
    x = value.detach().double().clone().requires_grad_()
    lp = log_prob(a, x)
    if mask is not None:
        lp = torch.where(mask, lp, torch.zeros((), dtype=lp.dtype))
    total = lp.sum(-1) * scale
    da, dx = torch.autograd.grad(total.sum() * g0, [a, x])
    return total.detach(), da, dx


def entropy(concentration: torch.Tensor) -> torch.Tensor:
    """dirichlet.py:122-130 in float64, summed over the rows (differentiable)."""
    a = concentration.double()
    a0 = a.sum(-1)
    C = a.shape[-1]
    h = torch.lgamma(a).sum(-1) - torch.lgamma(a0) - (C - a0) * torch.digamma(a0) - \
        ((a - 1.0) * torch.digamma(a)).sum(-1)
    return h.sum()


def normalise(g: torch.Tensor) -> torch.Tensor:
    """x = g / sum(g) with a float64 row sum, clamped as torch's sampler clamps, in float64."""
    g = g.double()
    return (g / g.sum(-1, keepdim=True)).clamp(FLT_MIN, ONE_BELOW)


class _Injected(torch.autograd.Function):
    """A Dirichlet draw with a supplied result x (backward: torch's _Dirichlet_backward), as
    tests/golden/make_golden.py does for Beta."""
    @staticmethod
    def forward(ctx, concentration, x):
        ctx.save_for_backward(x, concentration)
        return x.clone()

    @staticmethod
    def backward(ctx, grad):
        x, concentration = ctx.saved_tensors
        return _Dirichlet_backward(x, concentration, grad), None


def injected_draw(concentration: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """x [K, ..., C] as reparameterised draws of Dirichlet(concentration [..., C])."""
    return _Injected.apply(concentration.expand(x.shape), x)


class _InjectedStandardGamma(torch.autograd.Function):
    """torch._standard_gamma with a supplied result g (backward: torch._standard_gamma_grad)."""
    @staticmethod
    def forward(ctx, concentration, g):
        ctx.save_for_backward(concentration, g)
        return g.clone()

    @staticmethod
    def backward(ctx, grad):
        concentration, g = ctx.saved_tensors
        return grad * torch._standard_gamma_grad(concentration, g), None


def injected_gamma(concentration, rate, g):
    """g [K, ...] standard Gamma draws as draws of Gamma(concentration, rate) (gamma.py:80-88)."""
    return _InjectedStandardGamma.apply(concentration.expand(g.shape), g) / rate
