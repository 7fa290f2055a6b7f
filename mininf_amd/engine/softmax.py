"""
Softmax regression sites: Categorical(logits = X @ Theta) with a per-particle matrix Theta
[K, P, C], fused (``mi_softmax_linear_forward``; the model's matmul was deferred by
:mod:`mininf_amd.linear`). Such a site is planned as a row site -- an entry (site, (Theta,), labels,
mask) of the planner's categorical list whose record carries its launcher (``site.launcher``, run
by ``engine._rows._run_row_site`` under the row sites' one contract) -- so the ELBO plan,
``log_joint`` and ``LogLikelihoodLoss`` take it like a Categorical site: its speculative gradient
is dense in Theta, and it declines absorption like every row site.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _native as nat
from .. import data
from ..linear import put_back
from ..particles import SiteRecord
from ._operands import _collapse, _to_device
from ._rows import _buffers, _run_categorical


class _SoftmaxLauncher:
    """One ``mi_softmax_linear_forward`` site."""
    def __init__(self, site: SiteRecord, K: int, device: torch.device, value: torch.Tensor,
                 mask: Optional[torch.Tensor]) -> None:
        self.site, self.K, self.device = site, K, device
        self.X = site.linear_X
        self.N, self.P = self.X.shape
        self.value = value            # [N] int64 or float32 labels
        self.mask = mask              # [N] bool or None
        # device-resident minibatch read through its row index (mininf_amd.data): the dataset
        # columns of X and the labels, and the batch's rows
        self.batch: Optional["data._Batch"] = None
        self.X_src, self.value_src = self.X, value

    def describe(self, theta: torch.Tensor, g0: float) -> nat.SoftmaxLinear:
        L = nat.SoftmaxLinear()
        L.K, L.N, L.P, L.C = self.K, self.N, self.P, theta.shape[2]
        L.x = self.X_src.data_ptr()
        L.x_stride_i, L.x_stride_j = self.X_src.stride()
        L.theta = theta.data_ptr()
        L.theta_stride_k, L.theta_stride_j, L.theta_stride_c = theta.stride()
        if self.batch is not None:
            L.row_index = self.batch.rows.data_ptr()
        else:
            data.ensure_filled(self.X)
            data.ensure_filled(self.value)
        L.value = self.value_src.data_ptr()
        L.value_stride_i = self.value_src.stride(0)
        L.value_kind = nat.SOFTMAX_LABEL_INT64 if self.value_src.dtype == torch.int64 \
            else nat.SOFTMAX_LABEL_FLOAT32
        if self.mask is not None:
            L.mask = self.mask.data_ptr()
            L.mask_stride_i = self.mask.stride(0)
        L.grad_scale = g0
        L.site_scale = self.site.scale
        return L

    def run(self, params: Tuple[torch.Tensor], g0: float, flags: Optional[torch.Tensor] = None):
        """(total [K], (speculative dtheta [K, P, C] -- None where Theta needs none --,), no
        dvalue, flags [1]) for ``params`` = (Theta,)."""
        theta, = params
        need = theta.requires_grad
        device = self.device
        L = self.describe(theta, g0)
        if flags is not None:
            L.options |= nat.GROUP_FLAGS_ZEROED
        size = ctypes.c_size_t()
        lib = nat.lib()
        nat.check(lib.mi_softmax_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)),
                  "mi_softmax_linear_workspace_bytes")
        workspace, total, flags = _buffers(size.value, self.K, device, flags)
        dtheta = torch.empty(tuple(theta.shape), dtype=torch.float32, device=device) if need else None
        code = lib.mi_softmax_linear_forward(
            ctypes.byref(L), workspace.data_ptr(), size.value, total.data_ptr(), nat.ptr(dtheta),
            flags.data_ptr(), nat.stream_handle(device))
        if code == nat.MI_EUNSUPPORTED:
            return self._materialised(theta, g0, need, flags)
        nat.check(code, "mi_softmax_linear_forward")
        return total, (dtheta,), None, flags

    def _materialised(self, theta: torch.Tensor, g0: float, need: bool, flags: torch.Tensor):
        """The launch the library declined, as the row site on the materialised logits: what
        :meth:`run` returns."""
        X, value = self.X_src, self.value_src
        if self.batch is not None:
            rows = self.batch.rows.long()
            X, value = X[rows], value[rows]
        if value.is_floating_point():   # as plan_groups: -1 flags a non-integer label
            value = torch.where(value == value.trunc(), value, torch.full_like(value, -1.0))
        value = value.to(torch.int64).reshape(1, self.N).expand(self.K, self.N)
        mask = None if self.mask is None else self.mask.reshape(1, self.N).expand(self.K, self.N)
        with torch.no_grad():
            logits = torch.matmul(X, theta)
            total, dlogits, flags = _run_categorical(self.site, g0, logits, value, mask, need, flags)
            dtheta = torch.matmul(X.t(), dlogits) if need else None
        return total, (dtheta,), None, flags


def plan_softmax(site: SiteRecord, K: int, device: torch.device):
    """
    The row-site entry (site, (Theta,), labels, mask) of a Categorical site recorded on a deferred
    ``X @ Theta``, or None after materialising the logits as the model would have written them
    (``X @ Theta``, [K, N, C]) where the kernel cannot take the operands: the site is then the row
    site ``plan_groups`` makes of any Categorical.
    """
    theta = site.linear_theta
    X = site.linear_X
    shape = site.site_shape
    ok = theta is not None and theta.dtype == torch.float32 and theta.dim() == 3 and \
        theta.device == device and X.device == device and \
        theta.shape[2] <= nat.SOFTMAX_LINEAR_MAX_C
    if ok:
        value_t, _ = _to_device(site.tensors[-1], K, device, f"site '{site.name}'",
                                allow_constant=False)
        view = _collapse(value_t, K, shape)
        # (one particle -- LogLikelihoodLoss -- has no particle axis to depend on)
        ok = (view.sk == 0 or K == 1) and value_t.dtype in (torch.int64, torch.float32)
    if ok:
        value = view.tensor[0]   # [N]: the tracer records only unbatched values of shape (N,)
        mask = None
        if site.mask is not None:
            mask = site.mask.to(device).bool().expand(shape).reshape(-1)
        launcher = _SoftmaxLauncher(site, K, device, value, mask)
        xb, vb = data.lookup(X), data.lookup(view.tensor)
        if xb is not None and vb is not None and xb[0] is vb[0] and mask is None and \
                value.stride(0) == 1:
            launcher.batch = xb[0]
            launcher.X_src = xb[0].loader.columns[xb[1]]
            launcher.value_src = xb[0].loader.columns[vb[1]]
            if launcher.value_src.dtype != value.dtype:
                launcher.batch, launcher.X_src, launcher.value_src = None, X, value
        site.launcher = launcher
        return site, (theta,), value, mask
    put_back(site, K)
    return None
