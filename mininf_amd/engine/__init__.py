"""
ELBO engine: turns a :class:`~mininf_amd.particles.ParticleTrace` into HIP site-kernel launches and
wires them into autograd.

Per step (one ``EvidenceLowerBoundLoss.forward``):

1. sites that share their element space and a dense operand are grouped (at most 4 sites, 6
   operands) so the operand is streamed from HBM once and its gradient written once;
2. each group runs ``mi_group_forward`` (``include/mininf_amd.h``), which returns the per-particle
   totals ``T_k`` and -- speculatively, because the ELBO is linear in ``T`` -- the gradients of all
   operands, pre-multiplied by the upstream gradient the ELBO will send (``g0 = -1/K``);
3. in backward, ``mi_scale_rows`` leaves those buffers untouched when the upstream really is
   ``g0`` (every thread block exits after one comparison) and rescales them otherwise.

Gradient modes per operand: DENSE (one value per particle and element: written in the operand's
own layout), PARTICLE (one scalar per particle: reduced over elements inside the kernel).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

# Optional instrumentation (bench.py): an object with `pair(launcher) -> (start, stop)` returning
# torch.cuda.Event pairs (already created, or None) that mi_group_forward_deferred /
# mi_linear_forward_deferred record around the main site kernel of each launch, and
# `stamps(launcher) -> device address or None` of a (min start, max end) clock-stamp pair the
# kernel's workgroups fold their span into (mi_group.stamps).
KERNEL_TIMER = None

# _ElboPlan.fusions() of the last ELBO evaluation (EvidenceLowerBoundLoss.last_fusions): rebound by
# every elbo(), the same dict then updated by attach_optimizer
LAST_FUSIONS: Dict[str, int] = {}

# The layers. The two names above are defined first: the launchers and the held step read and
# write them on this module when they run (bench.py assigns KERNEL_TIMER here).
from .. import guide
from ..particles import ParticleTrace, SiteRecord
from ._operands import (FAMILY_CODES, _INTEGER_VALUED, _ONE_PARAMETER, _Operand, _View, _collapse,
                        _float, _to_device)
from ._groups import _QUERY_ADDRESS, _GroupLauncher, _SiteGroupFn
from ._rows import (_RowSiteFn, _run_categorical, _run_dirichlet, _run_mixture_normal,
                    _run_row_site)
from ._linear import _LinearLauncher, _LinearSiteFn
from ._held import (PendingGrad, _FUSED_ADAM_MAX_NUMEL, _PendingStep, _defer_step,
                    attach_optimizer, discard_pending_step, flush_pending_step, grad_meta,
                    pending_step, torch_function_flush)
from ._plan import (LogJoint, claim_group_draws, claim_linear_draws, fold_linear_priors,
                    fold_priors, plan_groups, plan_linear, release_unsafe_claims)
from ._absorb import EntropyFactor, _Absorbed, entropy_factors, plan_absorption
from ._elbo_plan import _ElboPlan, _elbo_workspace, _is_unit_seed


def log_joint(trace: ParticleTrace, g0: float, device: torch.device) -> LogJoint:
    """
    Launch the site kernels for every recorded site and return the per-particle log joint.
    """
    K = trace.K
    lazy, _ = _lazy_uses(trace)
    if lazy:   # per-particle upstream gradients need the draws themselves
        _materialize_draws(trace, lazy)
    linears = plan_linear(trace, g0, device)
    launchers, categorical = plan_groups(trace, g0, device)
    totals: List[torch.Tensor] = []
    pending: List[Tuple[str, dict, List[SiteRecord]]] = []
    for site, params, val, mask in categorical:
        holder: dict = {}
        totals.append(_RowSiteFn.apply(site, holder, g0, *params, val, mask))
        pending.append((site.family, holder, [site]))
    for linear in linears:
        holder = {}
        totals.append(_LinearSiteFn.apply(linear, holder, *linear.inputs()))
        pending.append(("linear", holder, linear.flag_sites))
    for launcher in launchers:
        holder = {}
        totals.append(_SiteGroupFn.apply(launcher, holder, *launcher.inputs()))
        pending.append(("group", holder, launcher.flag_sites))
    for _, value in trace.fallback:
        totals.append(value.to(device=device, dtype=torch.float32))
    if totals:
        total = totals[0]
        for extra in totals[1:]:
            total = total + extra
    else:
        total = torch.zeros(K, device=device)
    return LogJoint(total=total, pending=pending, checks=trace.checks)


class _ElboFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan: _ElboPlan, *inputs):  # type: ignore[override]
        ctx.plan = plan
        return plan.forward()

    @staticmethod
    def backward(ctx, u: torch.Tensor):  # type: ignore[override]
        return (None, *ctx.plan.backward(u))


def _materialize_draws(trace: ParticleTrace, draws) -> None:
    """
    Replace the placeholders of the given lazy draws in the trace's site tensors by the real
    draws (mi_normal_rsample), broadcast like the placeholders were.
    """
    for site in trace.sites:
        site.tensors = [t if guide.lazy_of(t) not in draws else
                        guide.lazy_of(t).materialize().expand(t.shape) for t in site.tensors]


def _lazy_uses(trace: ParticleTrace) -> Tuple[set, set]:
    """
    (all lazy draws in the trace's site tensors, those used where the kernels cannot compute
    them: linear / categorical / Dirichlet / mixture sites, or broadcast beyond the draw's own shape).
    """
    seen, bad = set(), set()
    for site in trace.sites:
        for t in site.tensors:
            lazy = guide.lazy_of(t)
            if lazy is None:
                continue
            seen.add(lazy)
            if site.linear_X is not None or site.gather_roles is not None or \
                    site.family in ("categorical", "dirichlet", "mixture_normal") or \
                    tuple(t.shape[1:]) != tuple(site.site_shape) or \
                    int(site.site_shape.numel()) != lazy.N:
                bad.add(lazy)
    return seen, bad


def elbo(trace: ParticleTrace, g0: float, device: torch.device, factors: List[EntropyFactor],
         entropy_scale: float, samples: Optional[Dict[str, torch.Tensor]] = None,
         flags: Optional[torch.Tensor] = None,
         step_words: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
         mirror: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, LogJoint]:
    """
    ``g0 * sum_k log p(x, z_k) - entropy_scale * H[factors]`` as one autograd node: the site
    kernels, the entropy and the reduction run in ``mi_group_forward`` / ``mi_elbo_forward``;
    backward is one ``mi_elbo_backward`` launch (plus the guide samplers' own backward).
    ``flags``: already-zeroed int32 validation words for the step, used when the plan's sites fit.
    ``step_words``: (counter, snapshot) generator words; the ELBO forward copies the counter to the
    snapshot and advances it. ``mirror``: host-mapped int32 words the ELBO forward copies the
    validation words into.
    """
    _, bad = _lazy_uses(trace)
    if bad:
        _materialize_draws(trace, bad)
    claims = claim_linear_draws(trace)
    linears = plan_linear(trace, g0, device, claims)
    while True:
        launchers, categorical = plan_groups(trace, g0, device)
        bad = {l.draw for l in launchers if l.draw is not None and not l.draw_supported()}
        if not bad:
            break
        _materialize_draws(trace, bad)
    launchers = fold_linear_priors(fold_priors(launchers), linears)
    release_unsafe_claims(linears, launchers, categorical)
    claim_group_draws(trace, launchers)
    guide.flush_draws()   # draws made while planning (materialised lazy draws)
    fallback = [value for _, value in trace.fallback]
    absorbed = plan_absorption(factors, samples, launchers, linears, categorical, fallback)
    plan = _ElboPlan(trace.K, g0, device, launchers, categorical, fallback, factors,
                     entropy_scale, linears, absorbed, flags, step_words, mirror)
    inputs = plan.inputs()
    # which autograd inputs are tensors (nn._Loss.backward maps the gradients to next_functions)
    plan.tensor_inputs = [isinstance(t, torch.Tensor) for t in inputs]
    loss = _ElboFn.apply(plan, *inputs)
    global LAST_FUSIONS
    LAST_FUSIONS = plan.fusions()
    pending: List[Tuple[str, dict, List[SiteRecord]]] = []
    for (site, _, _, _), holder in zip(categorical, plan.cat_holders):
        pending.append((site.family, holder, [site]))
    for linear, holder in zip(linears, plan.lin_holders):
        pending.append(("linear", holder, linear.flag_sites))
    for launcher, holder in zip(launchers, plan.holders):
        pending.append(("group", holder, launcher.flag_sites))
    joint = LogJoint(total=loss, pending=pending, checks=trace.checks, flags=plan.flags)
    if mirror is not None and plan.flags is not None and plan.flags.numel() <= mirror.numel():
        joint.mirror = mirror[:plan.flags.numel()]
    return loss, joint
