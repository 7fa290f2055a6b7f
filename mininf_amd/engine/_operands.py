"""
Operand views: how a site's tensors are described over the logical [K, N] element space of a
launch (strides, host constants, fused guide draws), and the family codes of ``mi_site``.
"""
from __future__ import annotations

import collections
import dataclasses
import functools
from typing import Optional, Tuple

import torch

from .. import _native as nat
from .. import graph, guide


FAMILY_CODES = {
    "normal": nat.NORMAL,
    "bernoulli_logits": nat.BERNOULLI_LOGITS,
    "bernoulli_probs": nat.BERNOULLI_PROBS,
    "beta": nat.BETA,
    "gamma": nat.GAMMA,
    "poisson": nat.POISSON,
    "inverse_gamma": nat.INVERSE_GAMMA,
    "exponential": nat.EXPONENTIAL,
    "laplace": nat.LAPLACE,
    "cauchy": nat.CAUCHY,
    "half_normal": nat.HALF_NORMAL,
    "half_cauchy": nat.HALF_CAUCHY,
    "log_normal": nat.LOG_NORMAL,
    "student_t": nat.STUDENT_T,
    "binomial": nat.BINOMIAL,
    "negative_binomial": nat.NEGATIVE_BINOMIAL,
}

# families with one parameter role: (parameter, -, value) in mi_site
_ONE_PARAMETER = ("bernoulli_logits", "bernoulli_probs", "poisson", "exponential", "half_normal",
                  "half_cauchy")
# families over the integers, whose values (and Binomial / NegativeBinomial total_count) may
# arrive as integer tensors
_INTEGER_VALUED = ("poisson", "binomial", "negative_binomial")


def _collapse(t: torch.Tensor, K: int, shape: torch.Size) -> "_View":
    """
    Describe a [K, *R] tensor (R broadcastable to ``shape``) over the logical [K, N] element space
    (N = numel(shape)). Per-particle scalars stay [K, 1] tensors with element stride 0 (their
    gradient is reduced in the kernel); broadcast and collapsible dims stay views; anything else is
    materialised by ``reshape``.
    """
    if t.dim() == 0:
        t = t.expand(K)
    R = tuple(t.shape[1:])
    N = int(torch.Size(shape).numel())
    if int(torch.Size(R).numel()) == 1:
        base = t.reshape(K, 1)
        return _View(base, base.stride(0), 0)
    if R == tuple(shape):   # already [K, *shape]: no broadcast view needed
        flat = t if len(R) == 1 else t.reshape(K, N)
        return _View(flat, flat.stride(0), flat.stride(1) if N > 1 else 1)
    full = t.reshape((K,) + (1,) * (len(shape) - len(R)) + R).expand((K,) + tuple(shape))
    flat = full.reshape(K, N)
    return _View(flat, flat.stride(0), flat.stride(1) if N > 1 else 1)


_DEVICE_CACHE: "collections.OrderedDict[Tuple, Tuple[torch.Tensor, torch.Tensor]]" = \
    collections.OrderedDict()


def _to_device(t: torch.Tensor, K: int, device: torch.device, what: str,
               allow_constant: bool = True) -> Tuple[Optional[torch.Tensor], Optional[float]]:
    """
    Bring a site tensor to the engine's device. Models written against the reference build
    distributions from Python numbers and CPU data (e.g. ``Beta(2, 2)``): such unbatched host values
    become kernel constants (scalars) or cached device copies (tensors, keyed on storage and
    version). Returns (tensor, None) or (None, constant).
    """
    if t.device == device:
        if allow_constant and not t.requires_grad and (t.dim() == 0 or t.stride(0) == 0):
            # a number of a distribution built in a captured step (mininf_amd.graph)
            value = graph.CONSTANT_VALUES.get(t.data_ptr())
            if value is not None and (t.dim() == 0 or t[0].numel() == 1):
                return None, value
        return t, None
    if t.device.type != "cpu":
        raise nat.NativeError(f"{what} lives on {t.device}, expected {device}")
    if t.requires_grad:
        raise nat.NativeError(f"{what} requires grad but lives on the CPU; move it to {device}")
    unbatched = t.dim() > 0 and t.stride(0) == 0
    base = t[0] if unbatched else t
    if allow_constant and unbatched and base.numel() == 1:
        return None, float(base.reshape(()))
    key = (base.data_ptr(), tuple(base.shape), tuple(base.stride()), base.dtype, base._version,
           str(device))
    hit = _DEVICE_CACHE.get(key)
    if hit is None:
        hit = (base, base.to(device))
        _DEVICE_CACHE[key] = hit
        while len(_DEVICE_CACHE) > 64:
            _DEVICE_CACHE.popitem(last=False)
    else:
        _DEVICE_CACHE.move_to_end(key)
    moved = hit[1]
    return (moved.expand((K,) + tuple(moved.shape)) if unbatched else moved), None


def _float(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise nat.NativeError(f"{what}: the HIP site kernels compute in float32 (the reference's "
                              f"default dtype); got {t.dtype}.")
    return t


@dataclasses.dataclass
class _View:
    tensor: Optional[torch.Tensor]  # autograd input ([K, N] view, or [K, 1] per-particle scalars)
    sk: int                         # element strides over the logical [K, N] space
    si: int
    constant: Optional[float] = None  # host scalar (e.g. the 2.0 of `Beta(2, 2)`): no operand
    draw: Optional[guide.LazyDraw] = None  # a guide draw computed inside the kernel (mi_draw)

    @functools.cached_property
    def key(self) -> Tuple:
        """Identity of the operand (views are not modified after construction: computed once)."""
        if self.constant is not None:
            return ("constant", self.constant)
        if self.draw is not None:
            return ("draw", id(self.draw))
        t = self.tensor
        return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), self.sk, self.si,
                t.requires_grad)

    @property
    def dense(self) -> bool:
        return self.constant is None and self.sk != 0 and self.si != 0

    @property
    def per_particle(self) -> bool:
        """One scalar per particle: the gradient is reduced over elements inside the kernel."""
        return self.constant is None and self.draw is None and self.tensor.shape[1] == 1 and \
            self.si == 0

    @property
    def requires_grad(self) -> bool:
        if self.draw is not None:
            return self.draw.loc.requires_grad or self.draw.scale.requires_grad
        return self.tensor.requires_grad


@dataclasses.dataclass
class _Operand:
    view: _View
    mode: int
    slot: int = -1
