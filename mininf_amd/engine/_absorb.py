"""
Guide factors in the ELBO kernels: the factors whose entropy ``mi_elbo_forward`` evaluates
(``mi_factor``) and the plan by which the ELBO backward absorbs a factor's draw.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _native as nat
from .. import guide, switches


@dataclasses.dataclass
class EntropyFactor:
    """
    A guide factor whose entropy the ELBO kernels evaluate (``mi_factor``): ``tensor`` is the
    autograd input -- Normal: the scale as [n] (stride 1, or any stride when n == 1); Beta: the
    interleaved [n, 2] concentration array; Gamma: the interleaved [n, 2] (concentration, rate). ``name`` / ``distribution`` identify the factor's
    draw in the samples (for absorbing the draw's backward).
    """
    family: int
    n: int
    tensor: torch.Tensor
    name: Optional[str] = None
    distribution: Optional[object] = None
    weight: float = 1.0   # mi_factor.weight: 1/W for a factor replicated on W data-sharded ranks


@dataclasses.dataclass(eq=False)
class _Absorbed:
    """
    A guide factor whose draw feeds only this ELBO's kernels: the ELBO backward computes the
    draw's backward, the entropy gradient and the guide transform's chain rule in one kernel and
    returns the gradients of the module's unconstrained parameters directly (``mi_factor`` with
    ``draw_kind``). ``uses``: (kind, launcher / linear index, operand index) with kind in
    "draw" (fused draw partials), "dense", "slot" (group gradients), "lin_theta", "lin_sigma".
    ``params``: per factor parameter (Normal loc, scale; Beta concentration1, concentration0) the
    unconstrained tensor and its MI_TRANSFORM, or None for a constant.
    """
    kind: int
    uses: List[Tuple[str, int, int]]
    params: List[Optional[Tuple[torch.Tensor, int]]]
    drawn: Optional[guide.Drawn] = None
    lazy: Optional[guide.LazyDraw] = None
    side_dgrad: Optional[torch.Tensor] = None   # Beta factors computed by a site launch (mi_side)
    saved: Optional[torch.Tensor] = None        # Beta: [n, 4] fp64 forward sums (mi_factor.saved)


_FACTOR_PARAMS = {nat.NORMAL: ("loc", "scale"), nat.BETA: ("concentration1", "concentration0")}


def _depends_on(tensors: Sequence[Optional[torch.Tensor]], target, limit: int = 20000) -> bool:
    """
    Whether autograd would route a gradient from any of ``tensors`` into the node ``target``.
    """
    if target is None:
        return False
    stack = [t.grad_fn for t in tensors if isinstance(t, torch.Tensor) and t.grad_fn is not None]
    seen = set()
    keep = []
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        if fn is target:
            return True
        seen.add(id(fn))
        keep.append(fn)
        if len(seen) > limit:
            return True   # too large to prove independence
        stack.extend(next_fn for next_fn, _ in fn.next_functions)
    return False


def _absorb_factor(factor: EntropyFactor, samples: Dict[str, torch.Tensor], launchers, linears,
                   categorical, fallback) -> Optional[_Absorbed]:
    """
    The absorption plan of one guide factor, or None when its draw's backward has to stay with
    autograd (the draw reaches the loss other than through the kernels' own operands, a parameter
    does not come straight from a ParameterizedDistribution, ...).
    """
    dist = factor.distribution
    if dist is None or factor.name is None or factor.name not in samples or \
            factor.family not in _FACTOR_PARAMS:
        return None   # Gamma draws keep their own backward (mi_gamma_rsample_backward)
    sources = getattr(dist, "_mininf_amd_sources", None) or {}
    params: List[Optional[Tuple[torch.Tensor, int]]] = []
    for pname in _FACTOR_PARAMS[factor.family]:
        source = sources.get(pname)
        if source is None:
            value = getattr(dist, pname, None)
            if isinstance(value, torch.Tensor) and value.requires_grad:
                return None   # derived some other way: autograd keeps it
            params.append(None)
            continue
        u, kind = source
        if tuple(u.shape) != tuple(dist.batch_shape) or u.dtype != torch.float32 or \
                not u.is_cuda or (u.numel() > 1 and not u.is_contiguous()):
            return None
        transform = nat.TRANSFORM_EXP if kind == "exp" else nat.TRANSFORM_NONE
        params.append((u, transform) if u.requires_grad else None)
    if all(p is None for p in params):
        return None
    sample = samples[factor.name]
    uses: List[Tuple[str, int, int]] = []
    lazy = guide.lazy_of(sample)
    if lazy is not None:
        if lazy.real is not None or factor.family != nat.NORMAL:
            return None
        for li, launcher in enumerate(launchers):
            for oi, op in enumerate(launcher.operands):
                if op.view.draw is lazy:
                    if op.mode != nat.GRAD_DENSE:
                        return None
                    uses.append(("draw", li, oi))
        if len(uses) != 1:
            return None
        return _Absorbed(nat.DRAW_PARTIALS, uses, params, lazy=lazy)
    drawn = guide.drawn_of(sample)
    if drawn is None or drawn.base._version != 0:
        return None
    if (drawn.family == guide.BETA_FAMILY) != (factor.family == nat.BETA):
        return None
    z = drawn.base
    N = drawn.N
    storage = z.untyped_storage().data_ptr()

    def shares(t) -> bool:
        return isinstance(t, torch.Tensor) and t.untyped_storage().data_ptr() == storage

    others: List[Optional[torch.Tensor]] = []
    for li, launcher in enumerate(launchers):
        for oi, op in enumerate(launcher.operands):
            v = op.view
            if v.draw is not None:
                others.extend([v.draw.loc, v.draw.scale])
                continue
            if v.tensor is None:
                continue
            if not shares(v.tensor):
                others.append(v.tensor)
                continue
            if v.tensor.data_ptr() != z.data_ptr():
                return None
            if op.mode == nat.GRAD_PARTICLE and N == 1 and v.sk == z.stride(0):
                uses.append(("slot", li, oi))
            elif op.mode == nat.GRAD_DENSE and launcher.N == N and v.sk == z.stride(0) and \
                    (v.si == z.stride(1) or N == 1):
                uses.append(("dense", li, oi))
            else:
                return None
    for j, linear in enumerate(linears):
        theta, sigma = linear.inputs()
        for which, t in (("lin_theta", theta), ("lin_sigma", sigma)):
            if t is None:
                continue
            if not shares(t):
                others.append(t)
                continue
            if t.data_ptr() != z.data_ptr():
                return None
            if which == "lin_theta" and linear.theta_grad and N == linear.P and \
                    tuple(t.stride()) == tuple(z.stride()):
                uses.append((which, j, -1))
            elif which == "lin_sigma" and linear.sigma_grad and N == 1 and \
                    t.stride(0) == z.stride(0):
                uses.append((which, j, -1))
            else:
                return None
    for _, params, value, _ in categorical:   # (the row site's parameters, value)
        for t in (*params, value):
            if shares(t):
                return None
            others.append(t)
    others.extend(fallback)
    if len(uses) > nat.MAX_SOURCES or _depends_on(others, z.grad_fn):
        return None
    return _Absorbed(nat.DRAW_SOURCES, uses, params, drawn=drawn)


def plan_absorption(factors: List[EntropyFactor], samples: Optional[Dict[str, torch.Tensor]],
                    launchers, linears, categorical, fallback) -> Dict[int, _Absorbed]:
    """
    Factor index -> absorption plan, for the factors whose draws' backward the ELBO kernels take
    over (``MININF_AMD_ABSORB=0`` disables it).
    """
    if not samples or not torch.is_grad_enabled() or \
            not switches.enabled("ABSORB"):
        return {}
    out: Dict[int, _Absorbed] = {}
    for index, factor in enumerate(factors):
        plan = _absorb_factor(factor, samples, launchers, linears, categorical, fallback)
        if plan is not None:
            out[index] = plan
    return out


def entropy_factors(approximation) -> Tuple[List[EntropyFactor], list]:
    """
    Split a factorised guide into factors whose entropy the ELBO kernels evaluate (Normal, Beta,
    Gamma) and the rest (whose entropy the loss evaluates by guide.entropy: the own kernel of the
    factor's family in guide.FAMILIES where it has one, else torch.distributions). With a factor in
    the rest the loss is no longer the fused node alone, so its gradients take autograd, never the
    direct-to-leaf paths.
    """
    from torch.distributions import Beta, Gamma, Normal

    from .. import guide
    fused: List[EntropyFactor] = []
    rest = []
    for name, factor in approximation.items():
        cls = type(factor)
        n = max(1, int(factor.batch_shape.numel()))
        if len(fused) < nat.MAX_FACTORS and cls is Normal and factor.scale.dtype == torch.float32 \
                and factor.scale.is_cuda and factor.scale.numel() == n:
            scale = factor.scale.reshape(n)
            if n > 1 and scale.stride(0) != 1:
                scale = scale.contiguous()
            fused.append(EntropyFactor(nat.NORMAL, n, scale, name, factor))
        elif len(fused) < nat.MAX_FACTORS and cls is Gamma and factor.concentration.is_cuda and \
                factor.concentration.dtype == torch.float32:
            # interleaved [n, 2] (concentration, rate), the Beta layout (one stack kernel)
            pair = torch.stack(torch.broadcast_tensors(factor.concentration, factor.rate), -1)
            fused.append(EntropyFactor(nat.GAMMA, n, pair.reshape(n, 2).contiguous(), name, factor))
        elif len(fused) < nat.MAX_FACTORS and cls is Beta:
            conc = guide.beta_concentration(factor, n)
            if conc.is_cuda:
                fused.append(EntropyFactor(nat.BETA, n, conc, name, factor))
            else:
                rest.append(factor)
        elif len(fused) < nat.MAX_FACTORS and guide.native_mvn(factor):
            # H = sum_i (0.5 + 0.5 log(2 pi) + log L_ii): the Normal entropy of diag(scale_tril),
            # read at its stride D + 1. The gradient 1 / L_ii comes back as a [D] tensor that
            # autograd scatters onto the diagonal (DiagonalBackward); the strictly lower entries
            # receive only the draw's gradient. No distribution is attached: the factor's draw
            # (mi_mvn_rsample) keeps its own backward, and a gradient routed through a view never
            # takes the direct-to-leaf paths (nn._accumulate_final_grads declines it).
            diagonal = factor.scale_tril.diagonal()
            fused.append(EntropyFactor(nat.NORMAL, int(diagonal.shape[0]), diagonal, name, None))
        else:
            rest.append(factor)
    return fused, rest
