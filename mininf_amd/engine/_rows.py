"""
Categorical and Dirichlet sites: one row of C entries per element, launched on their own
(``mi_categorical_forward`` / ``mi_dirichlet_forward``).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _native as nat
from ..particles import SiteRecord


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
    workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    total = torch.empty(K, dtype=torch.float32, device=device)
    if flags is None:
        flags = torch.empty(1, dtype=torch.int32, device=device)
    nat.check(lib.mi_categorical_forward(
        logits.data_ptr(), logits.stride(0), logits.stride(1), logits.stride(2), K, N, C,
        value.data_ptr(), value.stride(0), value.stride(1),
        None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(1),
        site.scale, g0, None if dlogits is None else dlogits.data_ptr(), workspace.data_ptr(),
        size.value, total.data_ptr(), flags.data_ptr(), nat.stream_handle(device)),
        "mi_categorical_forward")
    return total, dlogits, flags


class _CategoricalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, site: SiteRecord, holder: dict, g0: float, logits: torch.Tensor,
                value: torch.Tensor, mask: Optional[torch.Tensor]):  # type: ignore[override]
        total, dlogits, flags = _run_categorical(site, g0, logits, value, mask,
                                                 logits.requires_grad)
        holder["flags"] = flags
        ctx.dlogits = dlogits
        ctx.g0 = g0
        return total

    @staticmethod
    def backward(ctx, g):  # type: ignore[override]
        dlogits = ctx.dlogits
        if dlogits is None:
            return None, None, None, None, None, None
        K, N, C = dlogits.shape
        g = g.contiguous()
        nat.check(nat.lib().mi_scale_rows(dlogits.data_ptr(), N * C, 1, K, N * C, g.data_ptr(),
                                          ctx.g0, nat.stream_handle(g.device)), "mi_scale_rows")
        return None, None, None, dlogits, None, None


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
    workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    total = torch.empty(K, dtype=torch.float32, device=device)
    if flags is None:
        flags = torch.empty(1, dtype=torch.int32, device=device)
    nat.check(lib.mi_dirichlet_forward(
        conc.data_ptr(), conc.stride(0), conc.stride(1), conc.stride(2), K, N, C,
        value.data_ptr(), value.stride(0), value.stride(1), value.stride(2),
        None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(1),
        site.scale, g0, nat.ptr(dconc), nat.ptr(dvalue), workspace.data_ptr(), size.value,
        total.data_ptr(), flags.data_ptr(), nat.stream_handle(device)), "mi_dirichlet_forward")
    return total, dconc, dvalue, flags


class _DirichletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, site: SiteRecord, holder: dict, g0: float, conc: torch.Tensor,
                value: torch.Tensor, mask: Optional[torch.Tensor]):  # type: ignore[override]
        total, dconc, dvalue, flags = _run_dirichlet(
            site, g0, conc, value, mask, (conc.requires_grad, value.requires_grad))
        holder["flags"] = flags
        ctx.grads = (dconc, dvalue)
        ctx.g0 = g0
        return total

    @staticmethod
    def backward(ctx, g):  # type: ignore[override]
        g = g.contiguous()
        for grad in ctx.grads:
            if grad is not None:
                K, N, C = grad.shape
                nat.check(nat.lib().mi_scale_rows(grad.data_ptr(), N * C, 1, K, N * C,
                                                  g.data_ptr(), ctx.g0,
                                                  nat.stream_handle(g.device)), "mi_scale_rows")
        return None, None, None, ctx.grads[0], ctx.grads[1], None


def _run_row_site(site: SiteRecord, g0: float, param: torch.Tensor, value: torch.Tensor,
                  mask: Optional[torch.Tensor], flags: Optional[torch.Tensor] = None):
    """A categorical or Dirichlet site's launch: (total, dparameter, dvalue, flags)."""
    if site.family == "dirichlet":
        return _run_dirichlet(site, g0, param, value, mask,
                              (param.requires_grad, value.requires_grad), flags)
    total, dlogits, flags = _run_categorical(site, g0, param, value, mask, param.requires_grad,
                                             flags)
    return total, dlogits, None, flags
