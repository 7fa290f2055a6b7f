"""
LowRankMultivariateNormal site densities on the HIP kernels ``mi_lowrank_site_forward`` and
``mi_lowrank_site_backward`` (``csrc/lowrank_site.hip``).

Replaces ``LowRankMultivariateNormal.log_prob`` (torch ``lowrank_multivariate_normal.py:203-212``,
with ``_batch_lowrank_mahalanobis`` and ``_batch_lowrank_logdet``) for factor-analysis and
probabilistic-PCA likelihoods: rows ``x[N, D]`` under one ``(loc, cov_factor, cov_diag)`` per
particle. The forward keeps ``coef = C^-1 W^T (x - loc) / d`` (as two products with ``L^-1``, formed
in fp64 from ``_capacitance_tril``) and the backward gives the gradients
in closed form (``include/mininf_amd.h`` has the formulas), the whole derivative with respect to
cov_factor and cov_diag: nothing flows into the constructor's capacitance product and Cholesky.

The density is an ``autograd.Function`` with a vmap rule: inside the particle trace
(``torch.func.vmap`` over particles) it launches once for all particles on the physical tensors.
"""
from __future__ import annotations

import ctypes
import math
import sys
from typing import Optional, Tuple

import torch
from torch.distributions import LowRankMultivariateNormal
from torch.overrides import TorchFunctionMode

from . import _native as nat
from . import mvn, switches

_LAUNCHES = 0


def launches() -> int:
    """Native forward launches (``mi_lowrank_site_forward`` calls) since import."""
    return _LAUNCHES


def why_not(distribution) -> Optional[str]:
    """Why ``distribution``'s density stays on torch, or None when it runs on the kernels."""
    if type(distribution) is not LowRankMultivariateNormal:
        return "type"   # a subclass may override log_prob
    loc, W, d, L = _operands(distribution)
    if any(t.dtype != torch.float32 for t in (loc, W, d, L)):
        return "dtype"
    if not 1 <= int(W.shape[-1]) <= nat.LOWRANK_MAX_R:
        return "rank"
    if not 1 <= int(W.shape[-2]) <= nat.LOWRANK_SITE_MAX_D:
        return "size"
    if W.dim() != 2 or d.dim() != 1 or L.dim() != 2 or loc.dim() != 1:
        return "row batch"   # one factor per particle: per-row parameters are torch's
    if any(t.device.type != "cuda" for t in (loc, W, d, L)):
        return "host"
    if not switches.enabled("LOWRANK_SITE"):
        return "switch"
    return None


def enabled(distribution) -> bool:
    """Whether ``distribution``'s density runs on the kernels: exactly LowRankMultivariateNormal,
    float32 parameters on the device, one factor per particle (no row batch), R <=
    MI_LOWRANK_MAX_R, D <= MI_LOWRANK_SITE_MAX_D, and the switch LOWRANK_SITE on."""
    return why_not(distribution) is None


class ConstructorCholesky(TorchFunctionMode):
    """
    Sends the ``torch.linalg.cholesky`` of LowRankMultivariateNormal's constructor
    (lowrank_multivariate_normal.py:17-26, the R x R capacitance matrix) to ``mvn.cholesky_ex`` while
    a model is traced: mi_cholesky with torch's backward and a vmap rule, no host synchronisation,
    so a captured step can hold a model that constructs the distribution (rocSOLVER's potrf cannot
    be captured). Only that call -- found by the constructor's frame among the callers -- and only
    for a float32 device matrix within the kernel's rank, with the switch LOWRANK_SITE on; every
    other factorisation stays where it was. The returned ``info`` is not read: I + W^T diag(1 / d) W
    is positive definite whenever cov_diag > 0, which the parameter checks of the site assert.
    """
    _CODE = LowRankMultivariateNormal.__init__.__code__
    _DEPTH = 8   # the modes between the constructor and this one each add a frame

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is torch.linalg.cholesky and not kwargs and len(args) == 1 and \
                self._native(args[0]) and self._from_constructor():
            return mvn.cholesky_ex(args[0])[0]
        return func(*args, **(kwargs or {}))

    @staticmethod
    def _native(A) -> bool:
        return isinstance(A, torch.Tensor) and A.dtype == torch.float32 and A.is_cuda and \
            A.shape[-1] <= nat.LOWRANK_MAX_R and switches.enabled("LOWRANK_SITE") and \
            mvn.cholesky_supported(A)

    def _from_constructor(self) -> bool:
        frame = sys._getframe(2)
        for _ in range(self._DEPTH):
            if frame is None:
                return False
            if frame.f_code is self._CODE:
                return True
            frame = frame.f_back
        return False


def _operands(distribution: LowRankMultivariateNormal):
    return (distribution.loc, distribution._unbroadcasted_cov_factor,
            distribution._unbroadcasted_cov_diag, distribution._capacitance_tril)


def _sizes(value, loc, W, d, L) -> Tuple[int, int, int, int]:
    D, R = int(W.shape[-2]), int(W.shape[-1])
    if value.shape[-1] != D or loc.shape[-1] != D or d.shape[-1] != D or \
            tuple(L.shape[-2:]) != (R, R):
        raise ValueError(f"LowRankMultivariateNormal operands disagree: value "
                         f"{tuple(value.shape)}, loc {tuple(loc.shape)}, cov_factor "
                         f"{tuple(W.shape)}, cov_diag {tuple(d.shape)}, capacitance_tril "
                         f"{tuple(L.shape)}")
    K = max(int(t.shape[0]) for t in (value, loc, W, d, L))
    if any(int(t.shape[0]) not in (1, K) for t in (value, loc, W, d, L)):
        raise ValueError("LowRankMultivariateNormal operands disagree on the particle axis")
    return K, int(value.shape[1]), D, R


def _strided(t: torch.Tensor):
    """(contiguous tensor, its particle stride: 0 when the particles share it)."""
    t = t.contiguous()
    return t, (0 if t.shape[0] == 1 else t.stride(0))


def _workspace(K: int, N: int, D: int, R: int, device) -> torch.Tensor:
    size = ctypes.c_size_t()
    nat.check(nat.lib().mi_lowrank_site_workspace_bytes(K, N, D, R, ctypes.byref(size)),
              "mi_lowrank_site_workspace_bytes")
    return torch.empty(size.value, dtype=torch.uint8, device=device)


class _LowRankSiteLogProb(torch.autograd.Function):
    """(log_prob [K, N], coef [K, N, R]) of value [K or 1, N, D] under loc [K or 1, D], cov_factor
    [K or 1, D, R], cov_diag [K or 1, D] and capacitance_tril [K or 1, R, R]."""
    @staticmethod
    def forward(value, loc, W, d, L):  # type: ignore[override]
        global _LAUNCHES
        K, N, D, R = _sizes(value, loc, W, d, L)
        device = W.device
        (value, vk), (loc, lk), (W, wk), (d, dk), (L, tk) = (_strided(t) for t in
                                                             (value, loc, W, d, L))
        lp = torch.empty((K, N), dtype=torch.float32, device=device)
        coef = torch.empty((K, N, R), dtype=torch.float32, device=device)
        workspace = _workspace(K, N, D, R, device)
        nat.check(nat.lib().mi_lowrank_site_forward(
            value.data_ptr(), vk, D, loc.data_ptr(), lk, W.data_ptr(), wk, d.data_ptr(), dk,
            L.data_ptr(), tk, K, N, D, R, workspace.data_ptr(), workspace.numel(),
            lp.data_ptr(), coef.data_ptr(), nat.stream_handle(device)), "mi_lowrank_site_forward")
        _LAUNCHES += 1
        return lp, coef

    @staticmethod
    def setup_context(ctx, inputs, output):  # type: ignore[override]
        _, coef = output
        ctx.mark_non_differentiable(coef)
        ctx.save_for_backward(*inputs, coef)

    @staticmethod
    def backward(ctx, g, _gcoef):  # type: ignore[override]
        value, loc, W, d, L, coef = ctx.saved_tensors
        K, N, D, R = _sizes(value, loc, W, d, L)
        device = W.device
        shapes = [t.shape for t in (value, loc, W, d)]
        (value, vk), (loc, lk), (W, wk), (d, dk), (L, tk) = (_strided(t) for t in
                                                             (value, loc, W, d, L))
        g = g.to(torch.float32).expand(K, N)
        grads = [torch.empty((K, *shape[1:]), dtype=torch.float32, device=device) if needed
                 else None for shape, needed in zip(shapes, ctx.needs_input_grad)]
        workspace = _workspace(K, N, D, R, device)
        nat.check(nat.lib().mi_lowrank_site_backward(
            g.data_ptr(), g.stride(0), g.stride(1), value.data_ptr(), vk, D, loc.data_ptr(), lk,
            W.data_ptr(), wk, d.data_ptr(), dk, L.data_ptr(), tk, coef.data_ptr(), K, N, D, R,
            workspace.data_ptr(), workspace.numel(), *[nat.ptr(t) for t in grads],
            nat.stream_handle(device)), "mi_lowrank_site_backward")
        # a leaf the particles share: its [K, ...] gradient summed over them
        return (*[None if t is None else t.sum_to_size(shape) for t, shape in zip(grads, shapes)],
                None)

    @staticmethod
    def vmap(info, in_dims, value, loc, W, d, L):  # type: ignore[override]
        # every logical operand has a leading axis of size 1 (log_prob below): a particle-dependent
        # one gives it up for the particle axis, a shared one keeps it (size 1: stride 0). The
        # logical batch axes are the value's rows alone (enabled() declines a row batch of the
        # parameters), which log_prob has flattened into N.
        phys = [t.movedim(dim, 0).squeeze(1) if dim is not None and t.dim() > 1 and
                t.shape[1 if dim == 0 else 0] == 1 else t
                for t, dim in zip((value, loc, W, d, L), in_dims)]
        for t, rank in zip(phys, (3, 2, 3, 2, 3)):
            if t.dim() != rank or (t.shape[0] != 1 and t.shape[0] != info.batch_size):
                raise ValueError(f"_LowRankSiteLogProb under vmap takes operands with a leading "
                                 f"axis of size 1 and no row batch (lowrank_site.log_prob): got "
                                 f"{[tuple(t.shape) for t in (value, loc, W, d, L)]} batched "
                                 f"along {in_dims}")
        lp, coef = _LowRankSiteLogProb.apply(*phys)
        return (lp.unsqueeze(1), coef.unsqueeze(1)), (0, 0)


def log_prob(distribution: LowRankMultivariateNormal, value: torch.Tensor) -> torch.Tensor:
    """``distribution.log_prob(value)`` on the kernels (see :func:`enabled`): value [..., D] float32
    on the device, the result [...]. Inside the particle trace this is one launch for all
    particles."""
    loc, W, d, L = _operands(distribution)
    rows = value.shape[:-1]
    flat = value.to(torch.float32).reshape(1, math.prod(rows), value.shape[-1])
    lp, _ = _LowRankSiteLogProb.apply(flat, loc.unsqueeze(0), W.unsqueeze(0), d.unsqueeze(0),
                                      L.unsqueeze(0))
    return lp.reshape(rows)
