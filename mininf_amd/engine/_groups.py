"""
The group launcher: the ``mi_group`` descriptor of up to four sites that share their element space
and a dense operand, its launch (``mi_group_forward``) and its autograd node.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _native as nat
from .. import data, guide, switches
from .. import engine as _engine   # KERNEL_TIMER is read there at every launch
from ..particles import SiteRecord
from ._operands import FAMILY_CODES, _ONE_PARAMETER, _Operand, _View


# a non-null address for descriptors that are only queried (never dereferenced)
_QUERY_ADDRESS = 1 << 20


class _GroupLauncher:
    """
    Owns the ctypes descriptor of one site group and launches ``mi_group_forward``.
    """
    def __init__(self, K: int, N: int, g0: float, device: torch.device,
                 per_site: bool = False) -> None:
        self.K, self.N, self.g0, self.device = K, N, g0, device
        self.per_site = per_site  # also return each site's log density per particle (diagnostics)
        self.operands: List[_Operand] = []
        self.keys: Dict[Tuple, int] = {}
        self.sites: List[Tuple[SiteRecord, List[int], Optional[torch.Tensor]]] = []
        self.num_slots = 0
        # the fused draw's dloc / dscale partials stay in the workspace for the ELBO backward
        # (MI_GROUP_DRAW_PARTIALS); set by the ELBO plan when it absorbs the draw
        self.draw_partials = False
        self.exp_pending = None
        self.workspace: Optional[torch.Tensor] = None   # of the last run
        # Beta implicit-gradient factors carried as extra workgroups of this launch (mi_side):
        # (draws x [K, N], concentration [N, 2]) set by the ELBO plan; side_out is the [K, N, 2]
        # result of the last run, or None when the group's kernel cannot carry the job
        self.side: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.side_out: Optional[torch.Tensor] = None
        # a one-element prior site folded into this launch (mi_prior, fold_priors): (site, family
        # code, (constant, constant)); its validation word follows the group's own
        self.prior: Optional[Tuple[SiteRecord, int, Tuple[float, float]]] = None
        # a deferred one-element Normal guide draw this launch makes itself (mi_group.pdraw,
        # claim_group_draws): (the draw, the operand index that reads it)
        self.pdraw: Optional[Tuple[guide.PendingDraw, int]] = None
        self.made_pdraw = False   # the last launch made that draw (EvidenceLowerBoundLoss.last_fusions)

    @property
    def flag_sites(self) -> List[SiteRecord]:
        """The sites whose validation words this launch writes, in word order."""
        return [site for site, _, _ in self.sites] + ([self.prior[0]] if self.prior else [])

    def try_add(self, site: SiteRecord, views: List[_View], mask: Optional[_View]) -> bool:
        constants = [v.constant for v in views]
        views_in = views
        views = [v for v in views if v.constant is None]
        new = {v.key for v in views if v.key not in self.keys}
        if len(self.sites) >= nat.MAX_SITES or len(self.operands) + len(new) > nat.MAX_OPERANDS:
            return False
        draws = {id(op.view.draw) for op in self.operands if op.view.draw is not None} | \
            {id(v.draw) for v in views if v.draw is not None}
        if len(draws) > 1:   # one fused draw per group
            return False
        grad_on = torch.is_grad_enabled()
        slots = len({v.key for v in views if v.key not in self.keys and v.per_particle
                     and v.requires_grad and grad_on})
        if self.num_slots + slots > nat.MAX_SLOTS:
            return False
        indices = []
        for v in views:
            if v.key not in self.keys:
                mode, slot = nat.GRAD_NONE, -1
                if v.requires_grad and grad_on:
                    if v.per_particle:
                        mode, slot = nat.GRAD_PARTICLE, self.num_slots
                        self.num_slots += 1
                    else:
                        mode = nat.GRAD_DENSE
                self.keys[v.key] = len(self.operands)
                self.operands.append(_Operand(v, mode, slot))
            indices.append(self.keys[v.key])
        it = iter(indices)
        roles = [(-1, c) if c is not None else (next(it), 0.0) for c in constants]
        assert len(roles) == len(views_in)
        self.sites.append((site, roles, mask))
        return True

    def shares_dense_operand(self, views: List[_View]) -> bool:
        return any(v.key in self.keys and v.dense for v in views)

    def inputs(self, skip: Sequence[int] = ()) -> List[Optional[torch.Tensor]]:
        """
        Autograd inputs: one per operand, two (loc, scale) for a fused draw; None for the operands
        in ``skip`` (draws whose backward the ELBO absorbs).
        """
        out: List[Optional[torch.Tensor]] = []
        for index, op in enumerate(self.operands):
            if op.view.draw is not None:
                out.extend([None, None] if index in skip else [op.view.draw.loc,
                                                               op.view.draw.scale])
            else:
                out.append(None if index in skip else op.view.tensor)
        return out

    @property
    def draw(self) -> Optional["guide.LazyDraw"]:
        return next((op.view.draw for op in self.operands if op.view.draw is not None), None)

    def draw_supported(self) -> bool:
        """
        Python mirror of sites.hip draw_supported (plus the specialiser being enabled): whether
        the group's fused draw can run, or has to be materialised before launching.
        """
        if self.draw is None:
            return True
        if not switches.enabled("JIT") or self.N % 4 or self.N < 512:
            return False
        for op in self.operands:
            v = op.view
            if v.draw is not None or v.constant is not None:
                continue
            if v.si != 0 and v.si != 1:
                return False
        for _, _, mask in self.sites:
            if mask is not None and (mask.sk != 0 or mask.si not in (0, 1)):
                return False
        return True

    def describe(self, compute_grads: bool, fuse_exp: bool = False, query: bool = False):
        """
        The ctypes ``mi_group`` descriptor of this group plus freshly allocated dense gradient
        buffers (one per DENSE operand, None otherwise). ``fuse_exp``: a fused draw whose guide
        scale still waits for its exp transform reads the unconstrained parameter instead
        (``mi_draw.scale_exp``); otherwise the transform is launched first. ``query``: for a plan
        query only (``mi_group_prior_supported``): nothing is launched or allocated -- no pending
        transform or gather runs, and dense gradients get a placeholder address.
        """
        device = self.device
        K, N = self.K, self.N
        group = nat.Group()
        group.K, group.N = K, N
        group.num_sites = len(self.sites)
        group.num_operands = len(self.operands)
        group.num_slots = self.num_slots if compute_grads else 0
        group.compute_grads = int(compute_grads)
        group.grad_scale = self.g0
        grads: List[Optional[torch.Tensor]] = []
        for index, op in enumerate(self.operands):
            desc = group.operands[index]
            view = op.view
            grad = None
            mode = op.mode if compute_grads else nat.GRAD_NONE
            if view.draw is not None:
                d = view.draw
                desc.data = None
                desc.stride_k, desc.stride_i = N, 1
                desc.grad_mode = mode
                dw = group.draw
                dw.operand = index + 1
                dw.loc, dw.loc_stride = d.loc.data_ptr(), d.loc_s
                dw.scale, dw.scale_stride = d.scale.data_ptr(), d.scale_s
                source = guide.exp_source(d.scale) if fuse_exp else None
                if source is not None:
                    # the guide's deferred exp transform runs inside the site program, which
                    # writes the scale for the autograd of the transform (run() marks it filled)
                    self.exp_pending, dw.scale_exp = source
                elif not query:
                    guide.fill_exp(d.scale)   # a deferred transform runs before the kernel reads it
                # (a lazy draw has no injected noise)
                dw.seed, dw.step, dw.step_device, dw.stream_id, dw.particle_offset, \
                    dw.element_offset, _ = guide.philox_key(d.cfg, element=True)
                if mode == nat.GRAD_DENSE and self.draw_partials:
                    group.options |= nat.GROUP_DRAW_PARTIALS
                elif mode == nat.GRAD_DENSE and query:
                    dw.dloc = dw.dscale = _QUERY_ADDRESS
                elif mode == nat.GRAD_DENSE:
                    dloc = torch.empty(N, dtype=torch.float32, device=device)
                    dscale = torch.empty(N, dtype=torch.float32, device=device)
                    dw.dloc, dw.dscale = dloc.data_ptr(), dscale.data_ptr()
                    grad = (dloc, dscale)
                grads.append(grad)
                continue
            if not query:
                data.ensure_filled(view.tensor)   # a minibatch read directly: gather its rows
            desc.data = view.tensor.data_ptr()
            desc.stride_k, desc.stride_i = view.sk, view.si
            if mode == nat.GRAD_DENSE and query:
                desc.grad = _QUERY_ADDRESS
                desc.grad_stride_k, desc.grad_stride_i = view.sk, view.si
            elif mode == nat.GRAD_DENSE:
                sk, si = view.sk, view.si
                if (sk, si) in ((N, 1), (1, K)):
                    grad = torch.empty_strided((K, N), (sk, si), dtype=torch.float32, device=device)
                else:
                    grad = torch.empty((K, N), dtype=torch.float32, device=device)
                desc.grad = grad.data_ptr()
                desc.grad_stride_k, desc.grad_stride_i = grad.stride()
            desc.grad_mode = mode
            desc.slot = op.slot if mode == nat.GRAD_PARTICLE else 0
            grads.append(grad)
        for index, (site, roles, mask) in enumerate(self.sites):
            desc = group.sites[index]
            desc.family = FAMILY_CODES[site.family]
            if site.family in _ONE_PARAMETER:
                roles = [roles[0], (-1, 0.0), roles[1]]
            for q in range(3):
                desc.operand[q] = roles[q][0]
                desc.constant[q] = roles[q][1]
            if mask is not None:
                if not query:
                    data.ensure_filled(mask.tensor)
                desc.mask = mask.tensor.data_ptr()
                desc.mask_stride_k, desc.mask_stride_i = mask.sk, mask.si
            desc.scale = site.scale
            desc.extra = site.extra
        if self.prior is not None:
            pr = group.prior
            pr.present, pr.family = 1, self.prior[1]
            pr.constant[0], pr.constant[1] = self.prior[2]
            pr.scale = self.prior[0].scale
        if self.pdraw is not None and not self.pdraw[0].done:
            rec, index = self.pdraw
            if rec.source is None and not query:
                # no fused exp for this scale: a deferred transform runs before the program reads
                # it (as for the operand draw above)
                guide.fill_exp(rec.scale)
            rec.describe(group.pdraw)
            group.pdraw.operand = index + 1
        return group, grads

    def source(self) -> str:
        """
        The specialised kernel source the library generates for this group (diagnostics).
        """
        group, _ = self.describe(True)
        needed = ctypes.c_size_t()
        lib = nat.lib()
        nat.check(lib.mi_group_source(ctypes.byref(group), None, 0, ctypes.byref(needed)),
                  "mi_group_source")
        buf = ctypes.create_string_buffer(needed.value)
        nat.check(lib.mi_group_source(ctypes.byref(group), buf, needed.value, None),
                  "mi_group_source")
        return buf.value.decode()

    def compile_check(self, compute_grads: bool = True) -> str:
        """
        Compile the specialised kernel with hiprtc (no device needed); raises with the log.
        """
        group, _ = self.describe(compute_grads)
        log = ctypes.create_string_buffer(1 << 16)
        code = nat.lib().mi_group_compile_check(ctypes.byref(group), log, len(log))
        if code != 0:
            raise nat.NativeError("site program failed to compile:\n" + log.value.decode())
        return log.value.decode()

    def run(self, compute_grads: bool, flags: Optional[torch.Tensor] = None,
            defer: bool = False, ksum: bool = False):
        """
        Launch the group. ``flags``: an already-zeroed int32 slice (one word per site) to write the
        validation flags into, e.g. part of one buffer for every group of a step. ``defer``: leave
        the finalize reduction to the caller when the library allows (``self.reduce``, an
        ``mi_reduce``; None when the launch reduced itself). ``ksum``: the caller hands the
        reduction to the ELBO forward, so the launch may leave its site values summed over the
        particles (MI_GROUP_KSUM; ``self.reduce.ksum`` says whether it did).
        """
        device = self.device
        K, N = self.K, self.N
        self.exp_pending = None
        group, grads = self.describe(compute_grads, fuse_exp=True)
        if flags is None:
            flags = torch.empty(len(self.flag_sites), dtype=torch.int32, device=device)
        else:
            group.options |= nat.GROUP_FLAGS_ZEROED
        if ksum and defer and not self.per_site:
            group.options |= nat.GROUP_KSUM
        if self.prior is not None:   # its word after the group's own
            group.prior.flags = flags.data_ptr() + 4 * len(self.sites)
        size = ctypes.c_size_t()
        lib = nat.lib()
        nat.check(lib.mi_group_workspace_bytes(ctypes.byref(group), ctypes.byref(size)),
                  "mi_group_workspace_bytes")
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
        self.side_out = None
        if self.side is not None:
            x, conc = self.side
            supported = ctypes.c_int(0)
            nat.check(lib.mi_group_side_supported(ctypes.byref(group), ctypes.byref(supported)),
                      "mi_group_side_supported")
            if supported.value:
                Ks, Ns = x.shape
                out = torch.empty((Ks, Ns, 2), dtype=torch.float64, device=device)
                sd = group.side
                sd.x, sd.c1, sd.c1_stride = x.data_ptr(), conc.data_ptr(), 2
                sd.c0, sd.c0_stride = conc.data_ptr() + 4, 2
                sd.K, sd.N, sd.out = Ks, Ns, out.data_ptr()
                nat.check(lib.mi_group_workspace_bytes(ctypes.byref(group), ctypes.byref(size)),
                          "mi_group_workspace_bytes")
                if workspace.numel() < size.value:
                    workspace = torch.empty(size.value, dtype=torch.uint8, device=device)
                self.side_out = out
        total = torch.empty(K, dtype=torch.float32, device=device)
        site_lp = torch.empty((len(self.sites), K), dtype=torch.float64, device=device) \
            if self.per_site else None
        slot_grad = torch.empty((max(1, group.num_slots), K), dtype=torch.float32, device=device)
        start = stop = None
        group.stamps = None   # (a cached descriptor must not keep an earlier timing slot)
        if _engine.KERNEL_TIMER is not None:
            start, stop = _engine.KERNEL_TIMER.pair(self)
            group.stamps = _engine.KERNEL_TIMER.stamps(self)
        reduce = nat.Reduce()

        def launch():
            return lib.mi_group_forward_deferred(
                ctypes.byref(group), workspace.data_ptr(), size.value, total.data_ptr(),
                nat.ptr(site_lp), slot_grad.data_ptr(), flags.data_ptr(),
                None if start is None else start.cuda_event,
                None if stop is None else stop.cuda_event,
                nat.stream_handle(device), ctypes.byref(reduce) if defer else None)
        code = launch()
        if group.pdraw.operand and code == nat.MI_EUNSUPPORTED:
            # this launch does not make the per-particle draw: the draw's own launch first
            rec = self.pdraw[0]
            rec.launch()
            guide.take_draw(rec)
            group.pdraw = nat.Draw()
            code = launch()
        nat.check(code, "mi_group_forward_deferred")
        self.made_pdraw = bool(group.pdraw.operand)
        if group.pdraw.operand:
            guide.take_draw(self.pdraw[0])
        if self.exp_pending is not None:
            self.exp_pending.filled = True
            self.exp_pending = None
        self.reduce = reduce if defer and reduce.part else None
        self.workspace = workspace
        self.partials = None
        if group.options & nat.GROUP_DRAW_PARTIALS:
            offset, rows = ctypes.c_size_t(), ctypes.c_int64()
            nat.check(lib.mi_group_draw_partials(ctypes.byref(group), ctypes.byref(offset),
                                                 ctypes.byref(rows)), "mi_group_draw_partials")
            self.partials = (workspace.data_ptr() + offset.value, rows.value)
        return total, site_lp, grads, slot_grad, flags


class _SiteGroupFn(torch.autograd.Function):
    """
    Autograd node of one site group: forward returns T_k (fp32 [K]); backward returns the
    speculative gradients (rescaled only if the upstream differs from g0).
    """
    @staticmethod
    def forward(ctx, launcher: _GroupLauncher, holder: dict, *inputs):  # type: ignore[override]
        need = any(op.mode != nat.GRAD_NONE for op in launcher.operands)
        total, site_lp, grads, slot_grad, flags = launcher.run(need)
        holder["flags"] = flags
        holder["site_lp"] = site_lp
        ctx.launcher = launcher
        ctx.grads = grads
        ctx.slot_grad = slot_grad
        return total

    @staticmethod
    def backward(ctx, g: torch.Tensor):  # type: ignore[override]
        launcher: _GroupLauncher = ctx.launcher
        grads, slot_grad = ctx.grads, ctx.slot_grad
        if grads is None:  # a second backward through the same graph: recompute
            _, _, grads, slot_grad, _ = launcher.run(True)
        ctx.grads = None
        g = g.contiguous()
        device = g.device
        out: List[Optional[torch.Tensor]] = []
        if launcher.num_slots:
            # slot gradients are speculative too (pre-multiplied by g0): slot_grad[j, k] is row k
            nat.check(nat.lib().mi_scale_rows(slot_grad.data_ptr(), 1, launcher.K, launcher.K,
                                              launcher.num_slots, g.data_ptr(), launcher.g0,
                                              nat.stream_handle(device)), "mi_scale_rows")
        for op, grad in zip(launcher.operands, grads):
            if op.mode == nat.GRAD_DENSE:
                sk, si = grad.stride()
                nat.check(nat.lib().mi_scale_rows(grad.data_ptr(), sk, si, launcher.K, launcher.N,
                                                  g.data_ptr(), launcher.g0,
                                                  nat.stream_handle(device)), "mi_scale_rows")
                out.append(grad)
            elif op.mode == nat.GRAD_PARTICLE:
                out.append(slot_grad[op.slot].reshape(launcher.K, 1))
            else:
                out.append(None)
        return (None, None, *out)
