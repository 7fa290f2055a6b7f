"""
Row sites: the entries (site, parameters, value, mask) of the planner's categorical list, each
launched on its own. Categorical, Dirichlet and Normal-mixture sites have one row of C entries per
element (``mi_categorical_forward`` / ``mi_dirichlet_forward`` / ``mi_mixture_normal_forward``)
and their parameters are a tuple of [K, N, C] tensors: one for a Categorical or Dirichlet site,
three for a mixture. A site planned on a deferred predictor (engine.softmax, engine.gather) carries
its launcher, ``site.launcher``, whose ``run(params, g0, flags)`` returns what the three
``_run_*`` functions are brought to here: (total, the parameters' gradients, dvalue, flags).
:func:`_run_row_site` is that one launch for the ELBO plan and :class:`_RowSiteFn` the one
autograd function around it for ``log_joint``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _native as nat
from ..particles import SiteRecord


def _buffers(size: int, K: int, device: torch.device, flags: Optional[torch.Tensor]):
    """What every row-site launch writes: (a workspace of ``size`` bytes, total [K], ``flags`` or
    -- None given -- a validation word of the launch's own)."""
    workspace = torch.empty(max(1, size), dtype=torch.uint8, device=device)
    total = torch.empty(K, dtype=torch.float32, device=device)
    if flags is None:
        flags = torch.empty(1, dtype=torch.int32, device=device)
    return workspace, total, flags


def _run_categorical(site: SiteRecord, g0: float, logits: torch.Tensor, value: torch.Tensor,
                     mask: Optional[torch.Tensor], need: bool,
                     flags: Optional[torch.Tensor] = None):
    """
    Launch ``mi_categorical_forward``: (total [K], speculative dlogits or None, flags [1]).
    """
    K, N, C = logits.shape
    device = logits.device
    dlogits = torch.empty_like(logits) if need else None   # every entry written
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_categorical_workspace_bytes(K, N, ctypes.byref(size)),
              "mi_categorical_workspace_bytes")
    workspace, total, flags = _buffers(size.value, K, device, flags)
    nat.check(lib.mi_categorical_forward(
        logits.data_ptr(), logits.stride(0), logits.stride(1), logits.stride(2), K, N, C,
        value.data_ptr(), value.stride(0), value.stride(1),
        None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(1),
        site.scale, g0, None if dlogits is None else dlogits.data_ptr(), workspace.data_ptr(),
        size.value, total.data_ptr(), flags.data_ptr(), nat.stream_handle(device)),
        "mi_categorical_forward")
    return total, dlogits, flags


def _run_dirichlet(site: SiteRecord, g0: float, conc: torch.Tensor, value: torch.Tensor,
                   mask: Optional[torch.Tensor], need: Tuple[bool, bool],
                   flags: Optional[torch.Tensor] = None):
    """
    Launch ``mi_dirichlet_forward``: (total [K], speculative dconcentration / dvalue or None,
    flags [1]). ``need``: which of the two gradients to write.
    """
    K, N, C = conc.shape
    device = conc.device
    # contiguous [K, N, C], every entry written
    dconc = torch.empty((K, N, C), dtype=torch.float32, device=device) if need[0] else None
    dvalue = torch.empty((K, N, C), dtype=torch.float32, device=device) if need[1] else None
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_dirichlet_workspace_bytes(K, N, C, ctypes.byref(size)),
              "mi_dirichlet_workspace_bytes")
    workspace, total, flags = _buffers(size.value, K, device, flags)
    nat.check(lib.mi_dirichlet_forward(
        conc.data_ptr(), conc.stride(0), conc.stride(1), conc.stride(2), K, N, C,
        value.data_ptr(), value.stride(0), value.stride(1), value.stride(2),
        None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(1),
        site.scale, g0, nat.ptr(dconc), nat.ptr(dvalue), workspace.data_ptr(), size.value,
        total.data_ptr(), flags.data_ptr(), nat.stream_handle(device)), "mi_dirichlet_forward")
    return total, dconc, dvalue, flags


def _run_mixture_normal(site: SiteRecord, g0: float, params: Tuple[torch.Tensor, ...],
                        value: torch.Tensor, mask: Optional[torch.Tensor],
                        need: Tuple[bool, bool, bool, bool],
                        flags: Optional[torch.Tensor] = None):
    """
    Launch ``mi_mixture_normal_forward``: (total [K], speculative (dlogits, dloc, dscale) and
    dvalue or None, flags [1]). ``params``: logits, loc, scale as [K, N, C] views read through
    their own strides (0 where a tensor is particle- or row-constant); ``value`` [K, N].
    ``need``: which of the four gradients to write.
    """
    K, N, C = params[0].shape
    device = params[0].device
    # contiguous [K, N, C] / [K, N], every entry written
    dparams = tuple(torch.empty((K, N, C), dtype=torch.float32, device=device) if wanted else None
                    for wanted in need[:3])
    dvalue = torch.empty((K, N), dtype=torch.float32, device=device) if need[3] else None
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_mixture_normal_workspace_bytes(K, N, C, ctypes.byref(size)),
              "mi_mixture_normal_workspace_bytes")
    workspace, total, flags = _buffers(size.value, K, device, flags)
    strided = [x for t in params for x in (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))]
    nat.check(lib.mi_mixture_normal_forward(
        *strided, K, N, C, value.data_ptr(), value.stride(0), value.stride(1),
        None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(1),
        site.scale, g0, *[nat.ptr(g) for g in dparams], nat.ptr(dvalue), workspace.data_ptr(),
        size.value, total.data_ptr(), flags.data_ptr(), nat.stream_handle(device)),
        "mi_mixture_normal_forward")
    return total, dparams, dvalue, flags


def _run_row_site(site: SiteRecord, g0: float, params: Tuple[torch.Tensor, ...],
                  value: torch.Tensor, mask: Optional[torch.Tensor],
                  flags: Optional[torch.Tensor] = None):
    """A row site's launch: (total [K], the speculative gradients of ``params`` as a tuple -- None
    where none is needed --, dvalue or None, flags [1])."""
    if site.launcher is not None:   # planned on a deferred predictor (engine.softmax, .gather)
        return site.launcher.run(params, g0, flags)
    if site.family == "mixture_normal":
        return _run_mixture_normal(site, g0, params, value, mask,
                                   (*[p.requires_grad for p in params], value.requires_grad),
                                   flags)
    param, = params
    if site.family == "dirichlet":
        total, dconc, dvalue, flags = _run_dirichlet(
            site, g0, param, value, mask, (param.requires_grad, value.requires_grad), flags)
        return total, (dconc,), dvalue, flags
    total, dlogits, flags = _run_categorical(site, g0, param, value, mask, param.requires_grad,
                                             flags)
    return total, (dlogits,), None, flags


def _scale_rows(grad: torch.Tensor, g: torch.Tensor, g0: float) -> None:
    """``grad[k] *= g[k] / g0`` in place (``mi_scale_rows``; nothing is written where the upstream
    ``g`` [K], contiguous, is ``g0``) for a speculative gradient: K contiguous rows."""
    K, M = grad.shape[0], grad[0].numel()
    nat.check(nat.lib().mi_scale_rows(grad.data_ptr(), M, 1, K, M, g.data_ptr(), g0,
                                      nat.stream_handle(g.device)), "mi_scale_rows")


class _RowSiteFn(torch.autograd.Function):
    """A row site evaluated on its own (engine.log_joint): ``inputs`` are the entry's parameters,
    then its value and its mask."""
    @staticmethod
    def forward(ctx, site: SiteRecord, holder: dict, g0: float, *inputs):  # type: ignore[override]
        *params, value, mask = inputs
        total, dparams, dvalue, flags = _run_row_site(site, g0, tuple(params), value, mask)
        holder["flags"] = flags
        ctx.grads = (*dparams, dvalue)
        ctx.g0 = g0
        return total

    @staticmethod
    def backward(ctx, g):  # type: ignore[override]
        if any(grad is not None for grad in ctx.grads):   # (else nothing is launched)
            g = g.contiguous()
            for grad in ctx.grads:
                if grad is not None:
                    _scale_rows(grad, g, ctx.g0)
        return (None, None, None, *ctx.grads, None)
