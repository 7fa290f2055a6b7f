"""
Linear-predictor sites: Normal(X @ theta, sigma) / Bernoulli(logits = X @ theta) and the count
regressions Poisson(exp(X @ theta)) / Binomial(n, logits = X @ theta) /
NegativeBinomial(r, logits = X @ theta), fused (``mi_linear_forward``).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import torch

from .. import _native as nat
from .. import data, guide
from .. import engine as _engine   # KERNEL_TIMER is read there at every launch
from ..particles import SiteRecord
from ._operands import FAMILY_CODES, _View


class _LinearLauncher:
    """
    One ``mi_linear_forward`` site: the predictor ``X @ theta_k`` is evaluated inside the kernel
    (the model's matmul was deferred by :mod:`mininf_amd.linear`).
    """
    def __init__(self, site: SiteRecord, K: int, g0: float, device: torch.device,
                 theta: torch.Tensor, sigma: Optional[_View], value: _View,
                 mask: Optional[torch.Tensor], count: Optional[_View] = None) -> None:
        self.site, self.K, self.g0, self.device = site, K, g0, device
        self.X = site.linear_X
        self.N, self.P = self.X.shape
        # device-resident minibatch read through its row index (mininf_amd.data): the dataset
        # columns of X and the value, and the batch's rows
        self.batch: Optional["data._Batch"] = None
        self.X_src, self.value_src = self.X, None
        # Binomial / NegativeBinomial total_count: a constant, a [N] view, or (minibatch) the
        # dataset column the batch's rows index
        self.count, self.count_src = count, None
        self.theta = theta
        self.sigma = sigma
        self.sigma_input = None
        if sigma is not None and sigma.constant is None:
            self.sigma_input = sigma.tensor[:, :1]
        self.value = value
        self.mask = mask
        self.sites = [(site, None, mask)]   # flag layout: one word (+ the folded prior's)
        # a prior site over theta itself folded into this launch (mi_linear.prior,
        # fold_linear_priors): (site, family code, (constant, constant))
        self.prior: Optional[Tuple[SiteRecord, int, Tuple[float, float]]] = None
        # theta is a guide draw this launch makes itself (mi_linear.draw, guide.PendingDraw)
        self.draw: Optional[guide.PendingDraw] = None
        self.drew_theta = self.drew_rows = False   # what the last launch made itself
        # decided here, outside the autograd Function (whose forward runs with grad disabled)
        grad_on = torch.is_grad_enabled()
        self.theta_grad = grad_on and theta.requires_grad
        self.sigma_grad = grad_on and self.sigma_input is not None and \
            self.sigma_input.requires_grad

    @property
    def flag_sites(self) -> List[SiteRecord]:
        return [self.site] + ([self.prior[0]] if self.prior else [])

    def needs_grads(self) -> bool:
        return self.theta_grad or self.sigma_grad

    def inputs(self) -> List[Optional[torch.Tensor]]:
        return [self.theta, self.sigma_input]

    def describe(self, compute_grads: bool, draw_rows: bool = True,
                 query: bool = False, draw: bool = True) -> nat.Linear:
        """
        The ``mi_linear`` descriptor. ``query``: for a support query only -- a minibatch's rows
        are neither drawn nor taken (the descriptor reads the dataset's first rows).
        """
        L = nat.Linear()
        L.K, L.N, L.P = self.K, self.N, self.P
        L.family = FAMILY_CODES[self.site.family]
        L.x = self.X_src.data_ptr()
        L.x_stride_i, L.x_stride_j = self.X_src.stride()
        L.theta = self.theta.data_ptr()
        L.theta_stride_k, L.theta_stride_j = self.theta.stride()
        if self.batch is not None and query:
            L.value = self.value_src.data_ptr()
            L.value_stride_i = self.value_src.stride(0)
        elif self.batch is not None:
            # the batch's rows: drawn by this kernel when nothing has drawn them yet (one launch
            # less per step), else read through the row index
            R = self.batch.take_rows() if draw_rows else None
            if R is not None:
                L.rows = R
            else:
                L.row_index = self.batch.rows.data_ptr()
            L.value = self.value_src.data_ptr()
            L.value_stride_i = self.value_src.stride(0)
        else:
            data.ensure_filled(self.X)
            data.ensure_filled(self.value.tensor)
            L.value = self.value.tensor.data_ptr()
            L.value_stride_i = self.value.si
        if self.count is not None:
            if self.count.constant is not None:
                L.count_constant = self.count.constant
            elif self.batch is not None:
                L.count = self.count_src.data_ptr()
                L.count_stride_i = self.count_src.stride(0)
            else:
                data.ensure_filled(self.count.tensor)
                L.count = self.count.tensor.data_ptr()
                L.count_stride_i = self.count.si
        if self.mask is not None:
            L.mask = self.mask.data_ptr()
            L.mask_stride_i = self.mask.stride(0) if self.N > 1 else 1
        if self.sigma is not None:
            if self.sigma.constant is not None:
                L.scale_constant = self.sigma.constant
            else:
                L.scale = self.sigma_input.data_ptr()
                L.scale_stride_k = self.sigma_input.stride(0)
        L.grad_scale = self.g0
        L.site_scale = self.site.scale
        L.compute_grads = int(compute_grads)
        if self.prior is not None:
            pr = L.prior
            pr.present, pr.family = 1, self.prior[1]
            pr.constant[0], pr.constant[1] = self.prior[2]
            pr.scale = self.prior[0].scale
        if draw and self.draw is not None and not self.draw.done:
            self.draw.describe(L.draw)
        return L

    def run(self, compute_grads: bool, flags: Optional[torch.Tensor] = None,
            defer: bool = False):
        device = self.device
        L = self.describe(compute_grads)
        if flags is None:
            flags = torch.empty(len(self.flag_sites), dtype=torch.int32, device=device)
        else:
            L.options |= nat.GROUP_FLAGS_ZEROED
        size = ctypes.c_size_t()
        lib = nat.lib()
        if self.prior is not None:   # its word after the site's
            L.prior.flags = flags.data_ptr() + 4
        nat.check(lib.mi_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)),
                  "mi_linear_workspace_bytes")
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
        total = torch.empty(self.K, dtype=torch.float32, device=device)
        nslots = self.P + (1 if L.scale else 0)
        dslots = torch.empty((nslots, self.K), dtype=torch.float32, device=device) \
            if compute_grads else None
        start = stop = None
        L.stamps = None
        if _engine.KERNEL_TIMER is not None:
            start, stop = _engine.KERNEL_TIMER.pair(self)
            L.stamps = _engine.KERNEL_TIMER.stamps(self)
        reduce = nat.Reduce()

        def launch(L):
            return lib.mi_linear_forward_deferred(
                ctypes.byref(L), workspace.data_ptr(), size.value, total.data_ptr(),
                nat.ptr(dslots), flags.data_ptr(), None if start is None else start.cuda_event,
                None if stop is None else stop.cuda_event, nat.stream_handle(device),
                ctypes.byref(reduce) if defer else None)
        code = launch(L)
        if L.draw.operand and code == nat.MI_EUNSUPPORTED:
            # this launch shape does not draw theta: the guide's own draw first
            self.draw.launch()
            guide.take_draw(self.draw)
            zeroed, prior_flags = L.options & nat.GROUP_FLAGS_ZEROED, L.prior.flags
            # the batch is still pending (take_rows changes nothing), so this descriptor draws
            # the rows in the launch again; reading batch.rows here would launch the rows kernel
            # AND leave them to this launch: the loader counter would advance twice
            L = self.describe(compute_grads, draw=False)
            L.options |= zeroed
            L.prior.flags = prior_flags
            code = launch(L)
        elif L.draw.operand and code == 0:
            guide.take_draw(self.draw)
            self.drew_theta = True
        if L.rows.counter:
            if code == nat.MI_EUNSUPPORTED:   # this launch shape does not draw rows: draw first
                zeroed, prior_flags = L.options & nat.GROUP_FLAGS_ZEROED, L.prior.flags
                L = self.describe(compute_grads, draw_rows=False)
                L.options |= zeroed
                L.prior.flags = prior_flags
                code = launch(L)
            elif code == 0:
                self.batch.rows_taken()
                self.drew_rows = True
        nat.check(code, "mi_linear_forward_deferred")
        self.reduce = reduce if defer and reduce.part else None
        self.workspace = workspace   # holds the deferred partials
        return total, dslots, flags

    def grads(self, dslots: Optional[torch.Tensor]) -> List[Optional[torch.Tensor]]:
        if dslots is None:
            return [None, None]
        dtheta = dslots[:self.P].t() if self.theta_grad else None
        dsigma = dslots[self.P].reshape(self.K, 1) if self.sigma_grad else None
        return [dtheta, dsigma]


class _LinearSiteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, launcher: _LinearLauncher, holder: dict, theta, sigma):  # type: ignore
        total, dslots, flags = launcher.run(launcher.needs_grads())
        holder["flags"] = flags
        ctx.launcher, ctx.dslots = launcher, dslots
        return total

    @staticmethod
    def backward(ctx, g: torch.Tensor):  # type: ignore[override]
        launcher: _LinearLauncher = ctx.launcher
        dslots = ctx.dslots
        if dslots is None:
            return None, None, None, None
        ctx.dslots = None
        g = g.contiguous()
        # dslots[j, k] is row k of a [K, slots] view: rescale by g[k] / g0 unless equal
        nat.check(nat.lib().mi_scale_rows(dslots.data_ptr(), 1, launcher.K, launcher.K,
                                          dslots.shape[0], g.data_ptr(), launcher.g0,
                                          nat.stream_handle(g.device)), "mi_scale_rows")
        return (None, None, *launcher.grads(dslots))
