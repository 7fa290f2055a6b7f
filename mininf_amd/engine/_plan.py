"""
Planning: which launch evaluates each recorded site (linear sites, row sites, site groups), which
deferred guide draws those launches make themselves, which prior sites fold into another site's
launch, and the validation results of a step (:class:`LogJoint`).
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
from typing import Dict, List, Optional, Tuple

import torch

from .. import _native as nat
from .. import data, guide, particles, switches
from ..linear import put_back
from ..particles import ParticleTrace, SiteRecord
from ._groups import _QUERY_ADDRESS, _GroupLauncher
from ._held import flush_pending_step, pending_step
from ._linear import _LinearLauncher
from .softmax import plan_softmax
from .gather import plan_gather
from ._operands import FAMILY_CODES, _INTEGER_VALUED, _View, _collapse, _float, _to_device


def _storage(t: torch.Tensor) -> Optional[int]:
    return guide._storage_of(t)


def claim_linear_draws(trace: ParticleTrace) -> Dict[int, guide.PendingDraw]:
    """
    Deferred guide draws (:class:`guide.PendingDraw`) a linear site kernel makes itself
    (``mi_linear.draw``), by ``id`` of that site: the draw is the theta of exactly one linear site,
    and every other site tensor reading it is the [K, P] draw itself (e.g. the value of a prior
    over theta, which the linear launch evaluates too). Every other deferred draw is launched now,
    before planning reads anything.
    """
    if not guide._PENDING_DRAWS:
        return {}
    thetas: Dict[guide.PendingDraw, list] = collections.defaultdict(list)
    others: Dict[guide.PendingDraw, list] = collections.defaultdict(list)
    for site in trace.sites:
        if site.linear_X is not None and site.linear_theta is not None and \
                site.family != "categorical":   # (the softmax site's kernel does not draw)
            rec = guide.pending_draw(site.linear_theta)
            if rec is not None:
                thetas[rec].append(site)
        for t in site.tensors:
            rec = guide.pending_draw(t)
            if rec is not None:
                others[rec].append(t)
    claims = {}
    # one-element draws (a global parameter's K draws, e.g. the missing-observations model's mu)
    # stay pending for claim_group_draws: a fused-draw site program may make them itself
    keep = {id(rec) for rec in guide._PENDING_DRAWS.values() if rec.z.shape[-1] == 1}
    for rec, sites in thetas.items():
        z = rec.z
        if len(sites) == 1 and all(
                isinstance(t, torch.Tensor) and t.data_ptr() == z.data_ptr() and
                tuple(t.shape) == tuple(z.shape) and tuple(t.stride()) == tuple(z.stride())
                for t in others.get(rec, [])):
            claims[id(sites[0])] = rec
            rec.claimed = True
    claimed = set(map(id, claims.values())) | keep
    for key, rec in list(guide._PENDING_DRAWS.items()):
        if id(rec) not in claimed:
            del guide._PENDING_DRAWS[key]
            rec.launch()
    return claims


def claim_group_draws(trace: ParticleTrace, launchers: List["_GroupLauncher"]) -> None:
    """
    Deferred one-element Normal guide draws (a global parameter's K draws: the missing-
    observations model's ``mu``, examples/missing-observations.md:33-45) that a fused-draw site
    program makes itself (``mi_group.pdraw``): the draw is read only by that program, as one
    per-particle operand (its sites, and a prior folded into it). The program computes the draws
    from the same counter as ``mi_normal_rsample`` into a table of its own and writes them out, so
    the draw has no launch of its own. Unclaimed draws are launched by the caller's flush.
    """
    pending = [rec for rec in guide._PENDING_DRAWS.values()
               if not rec.claimed and not rec.done and rec.z.shape[-1] == 1]
    if not pending:
        return
    lib = nat.lib()
    for rec in pending:
        key = _storage(rec.z)
        # every site reading the draw must belong to one launcher (or be its folded prior)
        readers = []
        for site in trace.sites:
            if any(isinstance(t, torch.Tensor) and guide.pending_draw(t) is rec for t in site.tensors):
                readers.append(site)
        hosts = [(l, i) for l in launchers for i, op in enumerate(l.operands)
                 if op.view.tensor is not None and _storage(op.view.tensor) == key]
        if len(hosts) != 1:
            continue
        host, index = hosts[0]
        own = {id(site) for site, _, _ in host.sites}
        if host.prior is not None:
            own.add(id(host.prior[0]))
        if host.draw is None or host.operands[index].view.si != 0 or \
                any(id(site) not in own for site in readers):
            continue
        host.pdraw = (rec, index)
        group, _ = host.describe(True, query=True)
        if host.prior is not None:
            group.prior.flags = _QUERY_ADDRESS
        supported = ctypes.c_int(0)
        nat.check(lib.mi_group_pdraw_supported(ctypes.byref(group), ctypes.byref(supported)),
                  "mi_group_pdraw_supported")
        if supported.value:
            rec.claimed = True
        else:
            host.pdraw = None


def release_unsafe_claims(linears: List["_LinearLauncher"], launchers: List["_GroupLauncher"],
                          categorical) -> None:
    """
    Launch the claimed draws that a group or categorical launch also reads (a prior over theta
    that was not folded into the linear launch): those run before the linear sites.
    """
    drawn = {_storage(l.draw.z): l for l in linears if l.draw is not None}
    if not drawn:
        return
    read = set()
    for launcher in launchers:
        for op in launcher.operands:
            if op.view.tensor is not None:
                read.add(_storage(op.view.tensor))
    for site, params, val, _ in categorical:
        read.update(_storage(t) for t in (*params, val) if isinstance(t, torch.Tensor))
    for key in read & set(drawn):
        linear = drawn[key]
        linear.draw.launch()
        guide.take_draw(linear.draw)
        linear.draw = None


def plan_linear(trace: ParticleTrace, g0: float, device: torch.device,
                claims: Optional[Dict[int, guide.PendingDraw]] = None) -> List[_LinearLauncher]:
    """
    Launchers for the fused linear-predictor sites of a trace. A site whose operands the kernel
    cannot take (per-element sigma, particle-dependent values or counts, non-float32) gets its
    predictor materialised here as ``theta @ X.T`` (``exp`` of it for a Poisson site, whose role is
    the rate) and is planned like any other site.
    """
    K = trace.K
    out: List[_LinearLauncher] = []
    for site in trace.sites:
        if site.linear_X is None or site.family == "categorical":
            continue   # (a Categorical on X @ Theta: plan_groups, through plan_softmax)
        theta = site.linear_theta
        shape = site.site_shape
        launcher = None
        ok = theta is not None and theta.dtype == torch.float32 and theta.dim() == 2 and \
            theta.device == device and site.linear_X.device == device
        counted = site.family in ("binomial", "negative_binomial")
        if site.family in _INTEGER_VALUED and not (
                site.tensors[-1].dtype == torch.float32 and
                (not counted or site.tensors[0].dtype == torch.float32)):
            ok = False   # integer tensors: the site-group path converts them
        if ok:
            value_t, const = _to_device(_float(site.tensors[-1], site.name), K, device,
                                        f"site '{site.name}'", allow_constant=False)
            value = _collapse(value_t, K, shape)
            sigma = None
            if site.family == "normal":
                t, c = _to_device(_float(site.tensors[1], site.name), K, device,
                                  f"site '{site.name}'")
                sigma = _View(None, 0, 0, c) if c is not None else _collapse(t, K, shape)
                if sigma.constant is None and sigma.si != 0:
                    ok = False
            if value.sk != 0:
                ok = False
            count = None
            if counted:
                t, c = _to_device(site.tensors[0], K, device, f"site '{site.name}'")
                count = _View(None, 0, 0, c) if c is not None else _collapse(t, K, shape)
                if count.constant is None and (count.sk != 0 or count.tensor.requires_grad):
                    ok = False   # a total_count per particle (a latent dispersion)
            mask = None
            if site.mask is not None:
                mask = site.mask.to(device).bool().expand(shape).reshape(-1)
            if ok:
                launcher = _LinearLauncher(site, K, g0, device, theta, sigma, value, mask, count)
                xb, vb = data.lookup(site.linear_X), data.lookup(value.tensor)
                # (a per-row count joins a minibatch only as a column of the same loader)
                cb = data.lookup(count.tensor) if count is not None and count.constant is None \
                    else None
                count_ok = count is None or count.constant is not None or \
                    (cb is not None and xb is not None and cb[0] is xb[0] and count.si == 1)
                if xb is not None and vb is not None and xb[0] is vb[0] and mask is None and \
                        value.si == 1 and count_ok:
                    batch = xb[0]
                    launcher.batch = batch
                    launcher.X_src = batch.loader.columns[xb[1]]
                    launcher.value_src = batch.loader.columns[vb[1]]
                    if cb is not None:
                        launcher.count_src = batch.loader.columns[cb[1]]
        if launcher is None:
            put_back(site, K)   # the predictor as the model would have: theta @ X^T
            continue
        launcher.draw = (claims or {}).get(id(site))
        out.append(launcher)
    return out


@dataclasses.dataclass
class LogJoint:
    """
    Per-particle log joint of a trace plus the device-side validation results.
    """
    total: torch.Tensor                       # [K] fp32, differentiable
    pending: List[Tuple[str, dict, List[SiteRecord]]]
    checks: list
    flags: Optional[torch.Tensor] = None      # int32, one word per pending site, in order
    sticky: bool = False                      # flags are never zeroed by a replay (graph mode)
    mirror: Optional[torch.Tensor] = None     # host copy of `flags` the ELBO forward writes

    def flag_vector(self) -> Optional[torch.Tensor]:
        """
        All validation results of the step as one int64 device vector: one MI_FLAG_* word per
        kernel-evaluated site, then one 0/1 per deferred support / constraint check.
        """
        step = pending_step()
        if step is not None and (step.writes_flags or self.mirror is not None):
            # a held site launch finishing the ELBO writes the words, a held ELBO forward their
            # host mirror; a held ELBO forward with no mirror only reads them, and stays held for
            # the optimizer step (the validation read then waits for the site kernels alone)
            flush_pending_step()
        if self.flags is not None and not self.checks:
            return self.flags
        parts = []
        if self.flags is not None:
            parts.append(self.flags.to(torch.int64))
        else:
            for _, holder, _ in self.pending:
                parts.append(holder["flags"].reshape(-1).to(torch.int64))
        for _, ok in self.checks:
            parts.append((~ok.reshape(-1).bool()).any().reshape(1).to(torch.int64))
        if not parts:
            return None
        # host-evaluated checks (host values) join the device flags
        device = next((p.device for p in parts if p.device.type != "cpu"), parts[0].device)
        return torch.cat([p.to(device) for p in parts])

    def flag_count(self) -> int:
        return sum(len(sites) for _, _, sites in self.pending) + len(self.checks)

    def raise_from(self, values) -> None:
        """
        Raise the reference's errors (core.py:186-188 for values, torch validate_args for
        parameters) from host copies of :meth:`flag_vector`.
        """
        # every violation, then the first in model order (the reference raises at the first
        # sample statement that fails, core.py:142-189)
        found = []
        cursor = 0
        for kind, holder, sites in self.pending:
            for site in sites:
                bits = int(values[cursor])
                cursor += 1
                if bits & nat.FLAG_INTERNAL:
                    flush_pending_step()
                    raise RuntimeError(f"site '{site.name}': an in-kernel completion wait of its "
                                       "launch timed out (results of this step are invalid)")
                if bits & nat.FLAG_PARAM:
                    found.append((site.order, len(found), (
                        f"Expected parameters of distribution {site.description} for site "
                        f"'{site.name}' to satisfy their constraints, but found invalid values.")))
                elif bits & nat.FLAG_SUPPORT:
                    found.append((site.order, len(found),
                                  f"Parameter '{site.name}' is not in the support of "
                                  f"{site.description}."))
        for check, _ in self.checks:
            if int(values[cursor]):
                found.append((check.order, len(found), check.message))
            cursor += 1
        if found:
            flush_pending_step()   # the step's launches all run, as without a violation
            raise ValueError(min(found)[2])
        for check, _ in self.checks:
            if check.memo is not None:
                particles.memo_commit(check.memo)

    def raise_on_violation(self) -> None:
        """
        One host synchronisation for all validation flags of the step.
        """
        vector = self.flag_vector()
        if vector is not None:
            self.raise_from(vector.cpu().tolist())


def plan_groups(trace: ParticleTrace, g0: float, device: torch.device):
    """
    Prepare every recorded site for launch: categorical, Dirichlet and mixture sites as (site,
    parameters, value, mask) with the parameters a tuple of [K, N, C] tensors (logits |
    concentration | logits, loc, scale), sites on a deferred ``alpha[group]`` the same way with
    their tables and per-particle terms (engine.gather), and the other families packed into site groups sharing their element space and a dense operand.
    """
    K = trace.K
    groups: List[Tuple[torch.Size, _GroupLauncher]] = []
    categorical = []
    for site in trace.sites:
        if site.gather_roles is not None:
            entry = plan_gather(site, K, device)   # (None: materialised, grouped below)
            if entry is not None:
                categorical.append(entry)
                continue
        if site.linear_X is not None and site.family == "categorical":
            entry = plan_softmax(site, K, device)   # (None: materialised, the row site below)
            if entry is not None:
                categorical.append(entry)
                continue
        if site.linear_X is not None:
            continue   # planned by plan_linear
        if site.family == "categorical":
            logits, value = (_to_device(t, K, device, f"site '{site.name}'", False)[0]
                             for t in site.tensors)
            shape = site.site_shape
            C = logits.shape[-1]
            N = int(shape.numel())
            lg = _float(logits, site.name)
            lg = lg.reshape((K,) + (1,) * (len(shape) + 1 - (lg.dim() - 1)) + tuple(lg.shape[1:]))
            lg = lg.expand((K,) + tuple(shape) + (C,)).reshape(K, N, C).contiguous()
            if value.is_floating_point():
                # non-integer (or NaN) values are outside integer_interval(0, C - 1): -1 makes
                # the kernel flag them instead of the cast truncating them into the support
                value = torch.where(value == value.trunc(), value, torch.full_like(value, -1.0))
            val = _collapse(value.to(torch.int64), K, shape).tensor.expand(K, N)
            mask = None if site.mask is None else site.mask.to(device).bool().expand(shape) \
                .reshape(1, N).expand(K, N)
            categorical.append((site, (lg,), val, mask))
            continue
        if site.family == "dirichlet":
            # planned like a categorical site: (site, concentration, value, mask) as [K, N, C]
            # views (stride 0 along K for a particle-constant tensor), the mask as [K, N]
            conc, value = (_to_device(_float(t, site.name), K, device, f"site '{site.name}'",
                                      False)[0] for t in site.tensors)
            shape = site.site_shape
            C = conc.shape[-1]
            N = int(shape.numel())

            def rows(t: torch.Tensor) -> torch.Tensor:
                t = t.reshape((K,) + (1,) * (len(shape) + 1 - (t.dim() - 1)) + tuple(t.shape[1:]))
                return t.expand((K,) + tuple(shape) + (C,)).reshape(K, N, C)
            mask = None if site.mask is None else site.mask.to(device).bool().expand(shape) \
                .reshape(1, N).expand(K, N)
            categorical.append((site, (rows(conc),), rows(value), mask))
            continue
        if site.family == "mixture_normal":
            # (site, (logits, loc, scale), value, mask): the parameters as [K, N, C] views read
            # where they lie (stride 0 along K for a particle-constant tensor, along N for
            # components the rows share), the value and the mask as [K, N]
            *params, value = (_to_device(_float(t, site.name), K, device, f"site '{site.name}'",
                                         False)[0] for t in site.tensors)
            shape = site.site_shape
            C = max(int(p.shape[-1]) for p in params[1:])
            N = int(shape.numel())

            def rows(t: torch.Tensor) -> torch.Tensor:
                t = t.reshape((K,) + (1,) * (len(shape) + 1 - (t.dim() - 1)) + tuple(t.shape[1:]))
                return t.expand((K,) + tuple(shape) + (C,)).reshape(K, N, C)
            val = _collapse(value, K, shape).tensor.expand(K, N)
            mask = None if site.mask is None else site.mask.to(device).bool().expand(shape) \
                .reshape(1, N).expand(K, N)
            categorical.append((site, tuple(rows(p) for p in params), val, mask))
            continue
        shape = site.site_shape
        N = int(shape.numel())
        views = []
        for role, t in enumerate(site.tensors):
            is_value = role == len(site.tensors) - 1
            lazy = guide.lazy_of(t)
            if lazy is not None:   # exact-shape use, checked by _lazy_uses
                views.append(_View(None, N, 1, None, lazy))
                continue
            if site.family in _INTEGER_VALUED and not t.is_floating_point() and \
                    (is_value or (role == 0 and site.family != "poisson")):
                # integer counts and an integer total_count (exact in fp32 below 2^24); the
                # converted tensor takes no gradient (MI_GRAD_NONE)
                t = t.to(torch.float32)
            moved, constant = _to_device(_float(t, site.name), K, device, f"site '{site.name}'",
                                         allow_constant=not is_value)
            views.append(_View(None, 0, 0, constant) if constant is not None
                         else _collapse(moved, K, shape))
        mask = None
        if site.mask is not None:
            flat_mask = site.mask.to(device).bool().expand(shape).reshape(N)
            mask = _View(flat_mask, 0, flat_mask.stride(0) if N > 1 else 1)
        placed = False
        for group_shape, launcher in groups:
            if group_shape == shape and launcher.shares_dense_operand(views) and \
                    launcher.try_add(site, views, mask):
                placed = True
                break
        if not placed:
            launcher = _GroupLauncher(K, N, g0, device)
            launcher.try_add(site, views, mask)
            groups.append((shape, launcher))
    return [launcher for _, launcher in groups], categorical


_PRIOR_FAMILIES = ("beta", "normal", "gamma")


def fold_priors(launchers: List[_GroupLauncher]) -> List[_GroupLauncher]:
    """
    Fold one-element-per-particle prior sites into the launch of the site that reads the same
    per-particle tensor as its parameter (``mi_prior``; the README model's ``theta ~ Beta(2, 2)``
    under ``x ~ Bernoulli(theta)``, README.md:43-47): the prior's log density and its gradient are
    evaluated by that launch's particle-constant workgroups instead of a launch of their own.
    Only when the library's kernel for the host group carries it (``mi_group_prior_supported``)
    and both sites have the same scale; MININF_AMD_FOLD_PRIOR=0 disables it.
    """
    if not switches.enabled("FOLD_PRIOR"):
        return launchers
    out = list(launchers)
    lib = nat.lib()
    for prior in launchers:
        if len(prior.sites) != 1 or prior.N != 1 or prior.draw is not None or prior.per_site:
            continue
        site, roles, mask = prior.sites[0]
        if mask is not None or site.family not in _PRIOR_FAMILIES or roles[0][0] != -1 or \
                roles[1][0] != -1 or roles[2][0] < 0:
            continue
        value = prior.operands[roles[2][0]]
        for host in out:
            # the host's site 0 reads the prior's value as its per-particle parameter: a one-site
            # BCAST launch (the README model) or a fused-draw site program (the missing-
            # observations model's mu ~ Normal(0, 1) under z ~ Normal(mu, 1)); the library decides
            if host is prior or host.prior is not None or host.per_site:
                continue
            hsite, hroles, _ = host.sites[0]
            if hroles[0][0] < 0 or hsite.scale != site.scale:
                continue
            param = host.operands[hroles[0][0]]
            if param.view.key != value.view.key or param.mode != value.mode:
                continue
            host.prior = (site, FAMILY_CODES[site.family], (roles[0][1], roles[1][1]))
            group, _ = host.describe(True, query=True)
            group.prior.flags = _QUERY_ADDRESS
            supported = ctypes.c_int(0)
            nat.check(lib.mi_group_prior_supported(ctypes.byref(group), ctypes.byref(supported)),
                      "mi_group_prior_supported")
            if not supported.value:
                host.prior = None
                continue
            out.remove(prior)
            break
    return out


def fold_linear_priors(launchers: List[_GroupLauncher],
                       linears: List["_LinearLauncher"]) -> List[_GroupLauncher]:
    """
    Fold a prior site over a linear site's theta itself (every element, constant parameters: the
    regression's ``theta ~ Normal(0, 1)``, examples/minibatch.md:45-50) into the linear launch
    (``mi_linear.prior``): the first row block's workgroups evaluate it from the theta fragment
    they already hold, so the prior has no launch of its own. MININF_AMD_FOLD_PRIOR=0 disables it.
    """
    if not switches.enabled("FOLD_PRIOR") or not linears:
        return launchers
    out = list(launchers)
    lib = nat.lib()
    for prior in launchers:
        if len(prior.sites) != 1 or prior.draw is not None or prior.per_site:
            continue
        site, roles, mask = prior.sites[0]
        if mask is not None or site.family not in _PRIOR_FAMILIES or roles[0][0] != -1 or \
                roles[1][0] != -1 or roles[2][0] < 0:
            continue
        value = prior.operands[roles[2][0]]
        t = value.view.tensor
        for linear in linears:
            theta = linear.theta
            if linear.prior is not None or prior.N != linear.P or t is None or \
                    t.data_ptr() != theta.data_ptr() or (value.view.sk, value.view.si) != \
                    tuple(theta.stride()) or (value.mode == nat.GRAD_DENSE) != linear.theta_grad:
                continue
            linear.prior = (site, FAMILY_CODES[site.family], (roles[0][1], roles[1][1]))
            L = linear.describe(True, query=True)
            L.prior.flags = 1 << 20   # (any non-null word: only the launch shape is queried)
            supported = ctypes.c_int(0)
            nat.check(lib.mi_linear_prior_supported(ctypes.byref(L), ctypes.byref(supported)),
                      "mi_linear_prior_supported")
            if not supported.value:
                linear.prior = None
                continue
            out.remove(prior)
            break
    return out
