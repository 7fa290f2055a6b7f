"""
Fused ELBO: site groups + entropy + the scalar reduction in one autograd node.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Dict, List, Optional, Tuple

import torch

from .. import _native as nat
from .. import guide, switches
from ._absorb import EntropyFactor, _Absorbed
from ._held import _defer_step, flush_pending_step
from .gather import _GatherLauncher
from ._linear import _LinearLauncher
from ._rows import _run_row_site


_ELBO_WORKSPACE: Dict[Tuple[str, int], torch.Tensor] = {}
# workspaces replaced by a larger one: a captured hipGraph may still hold their addresses, so they
# are never freed
_ELBO_RETIRED: List[torch.Tensor] = []


def _elbo_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """
    Per-device workspace of ``mi_elbo_forward`` / ``mi_elbo_backward`` (its completion counters
    must start at zero and are left at zero by every launch, so the buffer is allocated and zeroed
    once and reused by every step, including captured graphs).
    """
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _ELBO_WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _ELBO_RETIRED.append(ws)
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        nat.check(nat.lib().mi_elbo_workspace_init(ws.data_ptr(), ws.numel(),
                                                   nat.stream_handle(device)),
                  "mi_elbo_workspace_init")
        _ELBO_WORKSPACE[key] = ws
    return ws


class _ElboPlan:
    """
    Everything one ELBO evaluation launches, in the order of the autograd inputs:
    site groups (their operand tensors), categorical / Dirichlet / mixture sites (logits |
    concentration | logits, loc, scale; value, mask), linear sites
    (theta, sigma), torch-evaluated sites (their [K] log densities) and the entropy factors (their
    parameter tensor, or -- absorbed -- the unconstrained parameters of both parameters).
    """
    def __init__(self, K: int, g0: float, device: torch.device, launchers, categorical,
                 fallback: List[torch.Tensor], factors: List[EntropyFactor],
                 entropy_scale: float, linears: Optional[List[_LinearLauncher]] = None,
                 absorbed: Optional[Dict[int, _Absorbed]] = None,
                 zeroed_flags: Optional[torch.Tensor] = None,
                 step_words: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                 mirror: Optional[torch.Tensor] = None) -> None:
        self.K, self.g0, self.device = K, g0, device
        self.zeroed_flags = zeroed_flags
        # (counter, snapshot): the generator words the ELBO forward advances (mi_elbo.step_counter)
        self.step_words = step_words
        # host-mapped copy of the validation words written by the ELBO forward (mi_elbo.flags_mirror)
        self.mirror = mirror
        self.recompute = False
        self.launchers = launchers
        self.categorical = categorical
        self.linears = linears or []
        self.lin_holders = [dict() for _ in self.linears]
        self.fallback = [v.to(device=device, dtype=torch.float32).reshape(K) for v in fallback]
        self.factors = factors
        self.entropy_scale = entropy_scale
        self.holders = [dict() for _ in launchers]
        self.cat_holders = [dict() for _ in categorical]
        self.flags: Optional[torch.Tensor] = None
        self.state = None
        self.tensor_inputs: Optional[List[bool]] = None
        self.deferred_count = 0
        self.absorbed = absorbed or {}
        # operands / linear inputs whose gradient an absorbed factor consumes
        self.skip_ops: Dict[int, set] = collections.defaultdict(set)
        self.skip_lin: set = set()
        for plan in self.absorbed.values():
            for kind, index, operand in plan.uses:
                if kind in ("draw", "dense", "slot"):
                    self.skip_ops[index].add(operand)
                    if kind == "draw":
                        launchers[index].draw_partials = True
                else:
                    self.skip_lin.add((kind, index))

    def inputs(self) -> List[Optional[torch.Tensor]]:
        out: List[Optional[torch.Tensor]] = []
        for li, launcher in enumerate(self.launchers):
            out.extend(launcher.inputs(self.skip_ops.get(li, ())))
        for _, params, val, mask in self.categorical:
            out.extend([*params, val, mask])
        for j, linear in enumerate(self.linears):
            theta, sigma = linear.inputs()
            out.append(None if ("lin_theta", j) in self.skip_lin else theta)
            out.append(None if ("lin_sigma", j) in self.skip_lin else sigma)
        out.extend(self.fallback)
        for index, f in enumerate(self.factors):
            plan = self.absorbed.get(index)
            if plan is None:
                out.append(f.tensor)
            else:
                out.extend(p[0] if p is not None else None for p in plan.params)
        return out

    def _describe(self, terms: List[torch.Tensor], buffers: List[torch.Tensor],
                  fill: bool = True) -> nat.Elbo:
        E = nat.Elbo()
        E.K = self.K
        E.g0 = self.g0
        E.entropy_scale = self.entropy_scale
        E.num_terms = len(terms)
        for j, t in enumerate(terms):
            E.terms[j] = t.data_ptr()
        E.num_factors = len(self.factors)
        for j, f in enumerate(self.factors):
            d = E.factors[j]
            d.family, d.n = f.family, f.n
            d.weight = f.weight
            # the entropy kernels read the parameters directly: a deferred exp transform no draw
            # kernel has written yet runs first (a no-op once a draw kernel wrote it; `fill`
            # False: the launch being described writes it)
            if fill:
                guide.fill_exp(f.tensor)
            base = f.tensor.data_ptr()
            if f.family in (nat.BETA, nat.GAMMA):
                d.param[0], d.param[1] = base, base + 4
                d.stride[0] = d.stride[1] = 2
            else:
                d.param[1] = base
                d.stride[1] = f.tensor.stride(0) if f.n > 1 else 0
        E.num_buffers = len(buffers)
        for j, b in enumerate(buffers):
            E.buffers[j] = b.data_ptr()
            E.buffer_len[j] = b.numel()
        return E

    def _describe_absorbed(self, E: nat.Elbo, results, lin_results) -> None:
        """Fill the absorbed draws' fields of the factor descriptors (after the site launches)."""
        for index, plan in self.absorbed.items():
            d = E.factors[index]
            f = self.factors[index]
            d.draw_kind = plan.kind
            for j, p in enumerate(plan.params):
                if p is not None:
                    d.transform[j] = p[1]
            if f.family == nat.NORMAL:
                loc = f.distribution.loc.reshape(f.n)
                if f.n > 1 and loc.stride(0) != 1:
                    loc = loc.contiguous()
                plan.loc = loc   # kept alive with the plan
                d.param[0] = loc.data_ptr()
                d.stride[0] = loc.stride(0) if f.n > 1 else 0
            if plan.kind == nat.DRAW_PARTIALS:
                _, li, _ = plan.uses[0]
                ptr, rows = self.launchers[li].partials
                d.partial[0], d.partial[1] = ptr, ptr + 4 * rows * f.n
                d.partial_rows = rows
                continue
            cfg = plan.drawn.cfg
            if f.family == nat.BETA:
                # the forward's per-element sums for this evaluation's backward, owned by the
                # plan so that interleaved evaluations never share them
                plan.saved = torch.empty(4 * f.n, dtype=torch.float64, device=self.device)
                d.saved = plan.saved.data_ptr()
                d.draws = plan.drawn.base.data_ptr()
                d.dgrad = nat.ptr(plan.side_dgrad if plan.side_dgrad is not None
                                  else plan.drawn.dgrad)
            else:
                # (the step word the ELBO backward reads)
                d.seed, d.step, d.step_device, d.stream_id, d.particle_offset, d.element_offset, \
                    d.eps = guide.philox_key(cfg, backward=True, element=True)
            d.num_sources = len(plan.uses)
            for s, (kind, li, oi) in enumerate(plan.uses):
                src = d.source[s]
                if kind == "dense":
                    grad = results[li][0][oi]
                    src.ptr = grad.data_ptr()
                    src.stride_k, src.stride_i = grad.stride()
                elif kind == "slot":
                    slot_grad = results[li][1]
                    src.ptr = slot_grad[self.launchers[li].operands[oi].slot].data_ptr()
                    src.stride_k, src.stride_i = 1, 0
                elif kind == "lin_theta":
                    src.ptr = lin_results[li].data_ptr()
                    src.stride_k, src.stride_i = 1, self.K
                else:   # lin_sigma
                    src.ptr = lin_results[li][self.linears[li].P].data_ptr()
                    src.stride_k, src.stride_i = 1, 0

    def forward(self) -> torch.Tensor:
        terms: List[torch.Tensor] = []
        buffers: List[torch.Tensor] = []
        results = []
        deferred: List[Tuple[nat.Reduce, torch.Tensor]] = []   # finalize reductions left to us
        fuse_env = switches.enabled("FUSE_REDUCE")
        ksum_env = switches.enabled("BCAST_KSUM")
        # one zeroed flag buffer for every site of the step, in `pending` order (categorical first)
        sizes = [1] * len(self.categorical) + [len(l.flag_sites) for l in self.linears] + \
            [len(l.flag_sites) for l in self.launchers]
        words = max(1, sum(sizes))
        zeroed, self.zeroed_flags = self.zeroed_flags, None   # zero only for the first forward
        if zeroed is not None and zeroed.numel() >= words:
            self.flags = zeroed[:words]
        else:
            self.flags = torch.zeros(words, dtype=torch.int32, device=self.device)
        cursor = len(self.categorical) + sum(len(l.flag_sites) for l in self.linears)
        # absorbed Beta draws whose implicit-gradient factors a site launch can carry (mi_side)
        side_jobs = [plan for plan in self.absorbed.values()
                     if plan.drawn is not None and plan.drawn.family == guide.BETA_FAMILY and
                     plan.drawn.dgrad is None and plan.drawn.conc is not None and
                     plan.drawn.base.numel() <= guide.BETA_DGRAD_MAX and
                     switches.enabled("BETA_SIDE")]
        for plan in side_jobs:
            plan.side_dgrad = None
        for li, (launcher, holder) in enumerate(zip(self.launchers, self.holders)):
            need = any(op.mode != nat.GRAD_NONE for op in launcher.operands)
            job = side_jobs[0] if side_jobs else None
            launcher.side = None if job is None else (
                job.drawn.base.reshape(self.K, job.drawn.N), job.drawn.conc)
            part = self.flags[cursor:cursor + len(launcher.flag_sites)]
            cursor += len(launcher.flag_sites)
            # Particle-summed site values (MI_GROUP_KSUM) only when the reductions will run inside
            # the ELBO forward -- decided here, before the launch, from what `fused` below is decided
            # from: the switch, at most MAX_REDUCE launches that can defer, and every absorbed Beta
            # factor's implicit-gradient factors at hand once this launch has carried its side job
            # (the launches that honour the option are those that carry one, mi_group_side_supported;
            # any other ignores it, and asking costs nothing).
            ksum = ksum_env and fuse_env and not launcher.per_site and \
                len(self.launchers) + len(self.linears) <= nat.MAX_REDUCE and \
                len(side_jobs) <= 1 and self._reduce_ok(assume=job)
            total, site_lp, grads, slot_grad, flags = launcher.run(need, part, defer=True,
                                                                   ksum=ksum)
            if launcher.reduce is not None:
                deferred.append((launcher.reduce, total))
            if job is not None and launcher.side_out is not None:
                job.side_dgrad = launcher.side_out
                side_jobs.pop(0)
            launcher.side = None
            holder["flags"], holder["site_lp"] = flags, site_lp
            terms.append(total)
            skip = self.skip_ops.get(li, set())
            if need:
                # speculative buffers the backward rescales when the upstream is not 1 (those an
                # absorbed factor consumes are scaled inside its own reduction instead)
                for oi, g in enumerate(grads):
                    if oi in skip:
                        continue
                    if isinstance(g, tuple):
                        buffers.extend(g)
                    elif g is not None:
                        buffers.append(g)
                if launcher.num_slots:
                    absorbed_slots = {launcher.operands[oi].slot for oi in skip
                                      if launcher.operands[oi].mode == nat.GRAD_PARTICLE}
                    if absorbed_slots:
                        buffers.extend(slot_grad[j:j + 1] for j in range(launcher.num_slots)
                                       if j not in absorbed_slots)
                    else:
                        buffers.append(slot_grad[:launcher.num_slots])
            results.append((grads, slot_grad, launcher.workspace))
        cat_results = []
        for j, ((site, params, val, mask), holder) in enumerate(zip(self.categorical,
                                                                    self.cat_holders)):
            total, dparams, dvalue, flags = _run_row_site(site, self.g0, params, val, mask,
                                                          self.flags[j:j + 1])
            holder["flags"] = flags
            terms.append(total)
            buffers.extend(g for g in (*dparams, dvalue) if g is not None)
            cat_results.append((dparams, dvalue))
        lin_results = []
        base = len(self.categorical)
        for j, (linear, holder) in enumerate(zip(self.linears, self.lin_holders)):
            words = len(linear.flag_sites)
            total, dslots, flags = linear.run(linear.needs_grads(),
                                              self.flags[base:base + words], defer=True)
            base += words
            if linear.reduce is not None:
                deferred.append((linear.reduce, total))
            holder["flags"] = flags
            terms.append(total)
            if dslots is not None:
                theta_out = ("lin_theta", j) in self.skip_lin
                sigma_out = ("lin_sigma", j) in self.skip_lin
                if not theta_out and not sigma_out:
                    buffers.append(dslots)
                else:
                    if not theta_out:
                        buffers.append(dslots[:linear.P])
                    if not sigma_out and dslots.shape[0] > linear.P:
                        buffers.append(dslots[linear.P:])
            lin_results.append(dslots)
        terms.extend(t.contiguous() for t in self.fallback)
        # The deferred reductions run inside the ELBO forward (their totals then leave `terms`)
        # unless there are too many, or a forward-absorbed Beta factor lacks its precomputed
        # implicit-gradient factors (mi_elbo.reduce); otherwise each runs as its own launch.
        fused = self._reduce_ok() and len(deferred) <= nat.MAX_REDUCE and fuse_env
        lib = nat.lib()
        self.deferred_count = len(deferred) if fused else 0
        self.ksum_count = sum(bool(job.ksum) for job, _ in deferred)
        if self.ksum_count and not fused:
            # cannot happen: the request above is made from the same facts as `fused` (a
            # particle-summed job has no per-particle values for mi_reduce_launch; an ELBO launch
            # too large to reduce its jobs itself handles such a job inside mi_elbo_forward)
            raise nat.NativeError("particle-summed site values without a fused reduction")
        if fused:
            reduced = {id(t) for _, t in deferred}
            terms = [t for t in terms if id(t) not in reduced]
        else:
            stream = nat.stream_handle(self.device)
            for job, _ in deferred:
                nat.check(lib.mi_reduce_launch(ctypes.byref(job), stream), "mi_reduce_launch")
            deferred = []
        if len(terms) > nat.MAX_TERMS:
            head = nat.MAX_TERMS - 1
            terms = terms[:head] + [torch.stack(terms[head:]).sum(0)]
        extra = buffers[nat.MAX_BUFFERS:]
        buffers = buffers[:nat.MAX_BUFFERS]
        E = self._describe(terms, buffers)
        self._describe_absorbed(E, results, lin_results)
        E.num_reduce = len(deferred)
        for j, (job, _) in enumerate(deferred):
            E.reduce[j] = job
        if self.step_words is not None and not self.recompute:
            E.step_counter = self.step_words[0].data_ptr()
            E.step_snapshot = self.step_words[1].data_ptr()
        if self.mirror is not None:
            E.flags = self.flags.data_ptr()
            E.flags_mirror = self.mirror.data_ptr()
            E.nflags = min(self.flags.numel(), self.mirror.numel())
        # The guide gradients of an upstream of exactly 1 (loss.backward() through nn._Loss's unit
        # seed) written by the forward when that leaves the backward nothing to do: the backward
        # then returns them without a launch (MI_ELBO_FINAL_GRADS).
        self.final = None
        if not self.recompute and not self.fallback and not extra and \
                switches.enabled("FINAL_GRADS"):
            complete = ctypes.c_int(0)
            nat.check(lib.mi_elbo_final_grads(ctypes.byref(E), ctypes.byref(complete)),
                      "mi_elbo_final_grads")
            if complete.value:
                self.final = self._factor_grads(E)
                E.options |= nat.ELBO_FINAL_GRADS
        size = ctypes.c_size_t()
        nat.check(lib.mi_elbo_workspace_bytes(ctypes.byref(E), ctypes.byref(size)),
                  "mi_elbo_workspace_bytes")
        ws = _elbo_workspace(self.device, size.value)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        guide.join_side()   # Beta implicit-gradient factors (mi_beta_dgrad) from the side stream
        stream = nat.stream_handle(self.device)

        def launch(adam):
            if adam is None:
                return lib.mi_elbo_forward(ctypes.byref(E), ws.data_ptr(), ws.numel(),
                                           loss.data_ptr(), stream)
            return lib.mi_elbo_forward_adam(ctypes.byref(E), ws.data_ptr(), ws.numel(),
                                            loss.data_ptr(), adam, stream)
        self.state = (E, results, cat_results, lin_results, extra, terms)
        # with the final gradients written, the launch is held for the optimizer step, which
        # then runs in its last block (mi_elbo_forward_adam). Everything E points to stays alive
        # until it runs: the backward drops self.state, and the deferred reductions' outputs
        # (written by this launch) are referenced nowhere else -- freed early, their memory would
        # be handed to the allocations made before the launch (the optimizer's own descriptor).
        keep = (self, E, ws, loss, self.state, self.final, deferred, buffers)
        if self.final is None or not _defer_step(launch, "mi_elbo_forward", self.final, keep,
                                                 self._elbo_adam(E), stream=(self.device, stream)):
            nat.check(launch(None), "mi_elbo_forward")
        return loss

    def _elbo_adam(self, E):
        """The adapter of the held ELBO forward: an mi_adam descriptor whose every tensor's
        gradient is one of the final gradients this launch writes -> the device pointer of the
        matching mi_elbo_adam (None: declined)."""
        final = self.final
        device = self.device

        def adapt(adam):
            if adam.num > nat.ELBO_ADAM_SLOTS:
                return None
            where = {}
            for f, grads in enumerate(final):
                if f not in self.absorbed:
                    continue
                for j, g in enumerate(grads):
                    if g is not None:
                        where[g.data_ptr()] = (f, j, g.numel())
            desc = nat.ElboAdam()
            desc.num, desc.maximize = adam.num, adam.maximize
            desc.lr, desc.beta1, desc.beta2 = adam.lr, adam.beta1, adam.beta2
            desc.eps, desc.weight_decay = adam.eps, adam.weight_decay
            for t in range(adam.num):
                T = adam.tensors[t]
                hit = where.get(T.grad)
                if hit is None or hit[2] != T.numel:
                    return None
                slot = desc.slots[t]
                slot.factor, slot.param = hit[0], hit[1]
                slot.value, slot.exp_avg, slot.exp_avg_sq = T.param, T.exp_avg, T.exp_avg_sq
                slot.step, slot.numel = T.step, T.numel
            ok = ctypes.c_int(0)
            nat.check(nat.lib().mi_elbo_adam_supported(ctypes.byref(E), ctypes.byref(desc),
                                                       ctypes.byref(ok)), "mi_elbo_adam_supported")
            return _elbo_adam_device(desc, device) if ok.value else None
        return adapt

    def fusions(self) -> Dict[str, int]:
        """
        Which fast paths this evaluation took (structural patterns the planner recognised; a model
        slightly off a pattern takes the general path, and this says so):
        folded_priors: prior sites evaluated by the launch of the site that reads their value
        (mi_prior); linear_theta_draws / linear_rows: linear launches that drew the guide's theta
        (mi_linear.draw) / their minibatch rows (mi_rows) themselves; fused_draws: Normal guide
        factors drawn in registers by the site programs (mi_draw); program_draws: one-element
        Normal guide factors drawn per particle by the site program that reads them (mi_group.pdraw,
        no draw launch); deferred_reductions: site
        reductions finished by the ELBO forward; final_grads: the forward wrote the guide
        gradients (no backward launch for loss.backward()); optimizer_step: the Adam step ran in the held launch's last block (no launch of its own);
        ``<family>_draws``: guide factors drawn by the native sampler of each family of
        guide.FAMILIES, and lowrank_entropies: LowRankMultivariateNormal guide factors whose
        entropy and its gradient the native kernel evaluated (mi_lowrank_entropy, called by the
        loss after this plan ran), as guide.counts() reports them; gathered_sites: sites on the model's own ``alpha[group]`` that
        this evaluation ran on a gather kernel (no [K, N] gather, no scatter-add);
        gathered_linear_sites: those of them with fixed effects, ``alpha[group] + X @ theta``, on
        mi_gather_linear_forward (no [K, N] product either); gathered_slope_sites: those of the
        gathered sites with slope terms ``beta[group] * z``, on mi_gather_slopes_forward.
        """
        # (a softmax-linear site's launcher counts nowhere here)
        gathered = [site.launcher for site, _, _, _ in self.categorical
                    if isinstance(site.launcher, _GatherLauncher) and site.launcher.launches > 0]
        return {
            "folded_priors": sum(l.prior is not None for l in self.launchers) +
            sum(l.prior is not None for l in self.linears),
            "linear_theta_draws": sum(l.drew_theta for l in self.linears),
            "linear_rows": sum(l.drew_rows for l in self.linears),
            "fused_draws": sum(p.kind == nat.DRAW_PARTIALS for p in self.absorbed.values()),
            "program_draws": sum(l.made_pdraw for l in self.launchers),
            "deferred_reductions": self.deferred_count,
            "particle_sums": getattr(self, "ksum_count", 0),
            "final_grads": int(getattr(self, "final", None) is not None),
            "optimizer_step": 0,   # set when the optimizer step joins the held launch
            # (lowrank_entropies: refreshed by the loss, which evaluates the rest's entropies)
            **guide.counts(),
            "gathered_sites": len(gathered),
            "gathered_linear_sites": sum(launcher.linear for launcher in gathered),
            "gathered_slope_sites": sum(launcher.slopes for launcher in gathered),
        }

    def _reduce_ok(self, assume=None) -> bool:
        """
        Whether the deferred reductions can join the ELBO forward: every forward-absorbed Beta
        factor has its implicit-gradient factors precomputed (its particle sums then move to the
        ELBO backward). ``assume``: a plan whose factors the next site launch computes as its side
        job.
        """
        for index, plan in self.absorbed.items():
            f = self.factors[index]
            if f.family != nat.BETA or plan.kind == nat.DRAW_PARTIALS or plan is assume:
                continue
            dgrad = plan.side_dgrad if plan.side_dgrad is not None else plan.drawn.dgrad
            if dgrad is None:
                return False
        return True

    def backward(self, u: torch.Tensor, hold: bool = False) -> List[Optional[torch.Tensor]]:
        if self.state is None:   # a second backward through the same graph: recompute
            # with this evaluation's generator step (the snapshot) and without advancing it again
            self.recompute = True
            for launcher in self.launchers:
                if launcher.draw is not None:
                    guide.use_snapshot(launcher.draw.cfg)
            self.forward()
        E, results, cat_results, lin_results, extra, _ = self.state
        self.state = None
        final, self.final = getattr(self, "final", None), None
        if final is not None and _is_unit_seed(u):
            # the forward wrote the gradients of exactly this upstream (MI_ELBO_FINAL_GRADS);
            # autograd reads them next (nn._accumulate_final_grads may hold them instead)
            if not hold:
                flush_pending_step()
            return self._outputs(results, cat_results, lin_results, None, final)
        device = self.device
        u = u.to(torch.float32).contiguous()
        dterm = torch.empty(1, dtype=torch.float32, device=device)
        fgrads = self._factor_grads(E)
        size = ctypes.c_size_t()
        lib = nat.lib()
        nat.check(lib.mi_elbo_workspace_bytes(ctypes.byref(E), ctypes.byref(size)),
                  "mi_elbo_workspace_bytes")
        ws = _elbo_workspace(device, size.value)
        nat.check(lib.mi_elbo_backward(ctypes.byref(E), u.data_ptr(), dterm.data_ptr(),
                                       ws.data_ptr(), ws.numel(), nat.stream_handle(device)),
                  "mi_elbo_backward")
        for buffer in extra:
            buffer.mul_(u)
        return self._outputs(results, cat_results, lin_results, dterm, fgrads)

    def _factor_grads(self, E) -> List[List[Optional[torch.Tensor]]]:
        """The guide factors' gradient outputs, their addresses written into E's factors."""
        device = self.device
        fgrads: List[List[Optional[torch.Tensor]]] = []
        for j, f in enumerate(self.factors):
            d = E.factors[j]
            plan = self.absorbed.get(j)
            if plan is not None:
                out_j: List[Optional[torch.Tensor]] = []
                for q, p in enumerate(plan.params):
                    if p is None:
                        d.grad[q] = None
                        out_j.append(None)
                        continue
                    grad = torch.empty(p[0].shape, dtype=torch.float32, device=device)
                    d.grad[q] = grad.data_ptr()
                    d.grad_stride[q] = 1
                    out_j.append(grad)
                fgrads.append(out_j)
                continue
            grad = torch.empty_like(f.tensor)
            base = grad.data_ptr()
            if f.family in (nat.BETA, nat.GAMMA):
                d.grad[0], d.grad[1] = base, base + 4
                d.grad_stride[0] = d.grad_stride[1] = 2
            else:
                d.grad[1] = base
                d.grad_stride[1] = grad.stride(0) if f.n > 1 else 1
            fgrads.append([grad])
        return fgrads

    def _outputs(self, results, cat_results, lin_results, dterm, fgrads
                 ) -> List[Optional[torch.Tensor]]:
        """The backward's gradients in the order of the autograd node's inputs."""
        out: List[Optional[torch.Tensor]] = []
        for li, (launcher, (grads, slot_grad, _)) in enumerate(zip(self.launchers, results)):
            skip = self.skip_ops.get(li, ())
            for oi, (op, grad) in enumerate(zip(launcher.operands, grads)):
                if op.view.draw is not None:
                    out.extend((None, None) if oi in skip or grad is None else grad)
                elif oi in skip:
                    out.append(None)
                elif op.mode == nat.GRAD_DENSE:
                    out.append(grad)
                elif op.mode == nat.GRAD_PARTICLE:
                    out.append(slot_grad[op.slot].reshape(launcher.K, 1))
                else:
                    out.append(None)
        for dparams, dvalue in cat_results:
            out.extend([*dparams, dvalue, None])
        for j, (linear, dslots) in enumerate(zip(self.linears, lin_results)):
            dtheta, dsigma = linear.grads(dslots)
            out.append(None if ("lin_theta", j) in self.skip_lin else dtheta)
            out.append(None if ("lin_sigma", j) in self.skip_lin else dsigma)
        out.extend(dterm.expand(self.K) for _ in self.fallback)
        for grads_j in fgrads:
            out.extend(grads_j)
        return out


def _is_unit_seed(u: torch.Tensor) -> bool:
    """Whether the upstream gradient is nn._Loss's cached device 1.0 (never written)."""
    from ..nn import _UNIT
    seed = _UNIT.get(u.device)
    return seed is not None and u.dtype == torch.float32 and u.numel() == 1 and \
        u.data_ptr() == seed.data_ptr()


# device copies of mi_elbo_adam descriptors (a captured step reads its copy on every replay, so
# copies are never freed; a process has a handful -- one per optimizer and model structure)
_ELBO_ADAM_COPIES: Dict[Tuple[int, bytes], torch.Tensor] = {}
_ELBO_ADAM_MAX_COPIES = 256


def _elbo_adam_device(desc, device: torch.device) -> Optional[int]:
    raw = bytes(desc)
    key = (device.index if device.index is not None else torch.cuda.current_device(), raw)
    buf = _ELBO_ADAM_COPIES.get(key)
    if buf is None:
        if len(_ELBO_ADAM_COPIES) >= _ELBO_ADAM_MAX_COPIES or \
                torch.cuda.is_current_stream_capturing():
            return None   # (no host-to-device copy inside a capture)
        buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        _ELBO_ADAM_COPIES[key] = buf
    return buf.data_ptr()
