"""
Predictive draws on the HIP samplers: the sites ``broadcast_samples`` (reference
``core.py:548-584``) has to simulate -- ``SampleTracer.sample`` draws them with the distribution's
own ``sample`` (``core.py:192-204``) -- come from the same counter-based Philox generator as the
guide draws (``mi_normal_rsample`` / ``mi_gamma_rsample`` / ``mi_beta_rsample`` and the predictive
kernels ``mi_predictive_sample`` / ``mi_predictive_categorical`` /
``mi_predictive_mixture_normal`` / ``mi_predictive_poisson``), so a
predictive run is reproducible from one seed and independent of how the samples are batched or
sharded.

Inside the vmapped predictive trace (:func:`mininf_amd.particles.broadcast_particles`) a site's
parameters are batched over the S samples. :class:`_DrawFn` carries a vmap rule: it receives the
physical ``[S, ...]`` parameters, broadcasts them to ``[S, *sample_shape, *batch_shape]`` as views
and draws all S samples in one launch. The generator counter of element j of sample s is
(seed, stream = the site's draw index, element s * M + j) with M the per-sample element count: a
value depends on (s, j, M) and not on S, so the first S' samples of a run are the run over those
S' samples alone; a shard that starts at a later sample has its own numbering from 0.

Drawn natively (exact type, float32 device parameters): Normal, Gamma, Beta, Bernoulli (probs or
logits, whichever the instance holds), Exponential, Laplace, Cauchy, HalfCauchy, HalfNormal,
LogNormal, Poisson, Categorical (up to 1024 categories) and MixtureSameFamily of a Categorical
over scalar Normal components (up to 1024 components). Everything else keeps torch's ``sample``
and torch's generator.
"""
from __future__ import annotations

import collections
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch.distributions import (Bernoulli, Beta, Categorical, Cauchy, Distribution, Exponential,
                                 Gamma, HalfCauchy, HalfNormal, Laplace, LogNormal,
                                 MixtureSameFamily, Normal, Poisson)
from torch.masked import MaskedTensor

from . import _native as nat

NORMAL, GAMMA, BETA = 0, 1, 2
POISSON, CATEGORICAL, MIXTURE_NORMAL = 3, 4, 5
# families of mi_predictive_sample: SAMPLE + its MI_PRED_* code
SAMPLE = 16
# stream ids of predictive draws: apart from the guide factors' (their factor index)
STREAM_BASE = 0x50000

_TWO_PARAMETERS = (NORMAL, GAMMA, BETA, SAMPLE + nat.PRED_LAPLACE, SAMPLE + nat.PRED_CAUCHY,
                   SAMPLE + nat.PRED_LOG_NORMAL)

# sites drawn natively since reset_counts(), by family name (guide.py counts its factors likewise)
_DRAWS: "collections.Counter[str]" = collections.Counter()


def native_draws() -> "collections.Counter[str]":
    """Family name -> sites drawn by the HIP samplers since the last :func:`reset_counts`."""
    return collections.Counter(_DRAWS)


def reset_counts(to: Optional["collections.Counter[str]"] = None) -> None:
    """Zero the counts of :func:`native_draws` (or set them to an earlier snapshot)."""
    _DRAWS.clear()
    if to is not None:
        _DRAWS.update(to)


def _params(distribution: Distribution) -> Optional[Tuple[int, Sequence[torch.Tensor]]]:
    cls = type(distribution)
    if cls is Normal:
        return NORMAL, (distribution.loc, distribution.scale)
    if cls is Gamma:
        return GAMMA, (distribution.concentration, distribution.rate)
    if cls is Beta:
        return BETA, (distribution.concentration1, distribution.concentration0)
    if cls is Bernoulli:
        # the parameter the instance was built from: the other one is a lazy property whose first
        # read launches the conversion
        if "probs" in distribution.__dict__:
            return SAMPLE + nat.PRED_BERNOULLI_PROBS, (distribution.__dict__["probs"],)
        return SAMPLE + nat.PRED_BERNOULLI_LOGITS, (distribution.__dict__["logits"],)
    if cls is Exponential:
        return SAMPLE + nat.PRED_EXPONENTIAL, (distribution.rate,)
    if cls is Laplace:
        return SAMPLE + nat.PRED_LAPLACE, (distribution.loc, distribution.scale)
    if cls is Cauchy:
        return SAMPLE + nat.PRED_CAUCHY, (distribution.loc, distribution.scale)
    if cls is HalfCauchy:
        return SAMPLE + nat.PRED_HALF_CAUCHY, (distribution.base_dist.scale,)
    if cls is HalfNormal:
        return SAMPLE + nat.PRED_HALF_NORMAL, (distribution.base_dist.scale,)
    if cls is LogNormal:
        return SAMPLE + nat.PRED_LOG_NORMAL, (distribution.base_dist.loc,
                                              distribution.base_dist.scale)
    if cls is Poisson:
        return POISSON, (distribution.rate,)
    if cls is Categorical:
        held = distribution.__dict__
        return CATEGORICAL, (held["logits"] if "logits" in held else held["probs"],)
    if cls is MixtureSameFamily and type(distribution.mixture_distribution) is Categorical and \
            type(distribution.component_distribution) is Normal:
        held = distribution.mixture_distribution.__dict__
        component = distribution.component_distribution
        return MIXTURE_NORMAL, (held["logits"] if "logits" in held else held["probs"],
                                component.loc, component.scale)
    return None


def supported(distribution: Distribution) -> bool:
    """Whether the HIP samplers draw this distribution (see the module docstring; float32 device
    parameters that are plain tensors)."""
    found = _params(distribution)
    if found is None:
        return False
    family, params = found
    if family == CATEGORICAL and not 1 <= params[0].shape[-1] <= nat.PRED_CATEGORICAL_MAX_C:
        return False
    if family == MIXTURE_NORMAL and not (
            isinstance(params[1], torch.Tensor) and params[1].dim() >= 1 and
            1 <= params[1].shape[-1] <= nat.PRED_CATEGORICAL_MAX_C):
        return False
    return all(isinstance(t, torch.Tensor) and not isinstance(t, MaskedTensor) and
               t.dtype == torch.float32 and _resident(t) for t in params)


def _resident(t: torch.Tensor) -> bool:
    return t.is_cuda


def _strided(t: torch.Tensor, S: int, M: int) -> Tuple[torch.Tensor, int, int]:
    """
    ``t`` (expanded to ``[S, ...]`` with M elements per sample) as a tensor to read in place and
    its element strides (stride_s, stride_j) over the logical ``[S, M]``. A view where
    ``.view(S, M)`` exists; otherwise one sample's elements are copied when the samples share them
    (stride_s = 0), and only a parameter that varies along both axes in a layout no stride pair
    describes is materialised at ``[S, M]``.
    """
    try:
        v = t.view(S, M)
    except RuntimeError:
        v = t[:1].reshape(1, M) if t.stride(0) == 0 else t.reshape(S, M)
    ss, sj = v.stride()
    return v, (0 if v.shape[0] == 1 else ss), (0 if M == 1 else sj)


def _single_stride(v: torch.Tensor, ss: int, sj: int, S: int, M: int) -> Tuple[torch.Tensor, int]:
    """The one element stride mi_normal / gamma / beta_rsample take (offset = (s * M + j) * stride)
    where (ss, sj) is of that form; a contiguous copy at stride 1 otherwise."""
    if S == 1:
        return v, sj
    if M == 1:
        return v, ss
    if ss == M * sj:
        return v, sj
    return v.expand(S, M).contiguous(), 1


def _launch(family: int, params: Sequence[Tuple[torch.Tensor, int, int]], S: int, M: int,
            seed: int, stream_id: int) -> torch.Tensor:
    """One launch drawing S * M values; each parameter is (tensor, stride_s, stride_j)."""
    device = params[0][0].device
    N = S * M
    out = torch.empty(N, dtype=torch.float32, device=device)
    stream = nat.stream_handle(device)
    lib = nat.lib()
    seed &= 0xFFFFFFFFFFFFFFFF
    if family >= SAMPLE:
        (a, a_ss, a_sj), (b, b_ss, b_sj) = params[0], params[-1]
        two = family in _TWO_PARAMETERS
        nat.check(lib.mi_predictive_sample(family - SAMPLE, a.data_ptr(), a_ss, a_sj,
                                           b.data_ptr() if two else None, b_ss, b_sj, S, M, seed,
                                           stream_id, out.data_ptr(), stream),
                  "mi_predictive_sample")
        return out
    if family == POISSON:
        rate, ss, sj = params[0]
        nat.check(lib.mi_predictive_poisson(rate.data_ptr(), ss, sj, S, M, seed, stream_id,
                                            out.data_ptr(), stream), "mi_predictive_poisson")
        return out
    (a, a_s), (b, b_s) = (_single_stride(*p, S, M) for p in params)
    if family == NORMAL:
        nat.check(lib.mi_normal_rsample(a.data_ptr(), a_s, b.data_ptr(), b_s, 1, N, seed, 0, None,
                                        stream_id, 0, 0, None, out.data_ptr(), stream),
                  "mi_normal_rsample")
    elif family == GAMMA:
        g = torch.empty(N, dtype=torch.float32, device=device)
        nat.check(lib.mi_gamma_rsample(a.data_ptr(), a_s, b.data_ptr(), b_s, 1, N, seed, 0, None,
                                       stream_id, 0, None, g.data_ptr(), out.data_ptr(), stream),
                  "mi_gamma_rsample")
    else:
        nat.check(lib.mi_beta_rsample(a.data_ptr(), a_s, b.data_ptr(), b_s, 1, N, seed, 0, None,
                                      stream_id, 0, None, out.data_ptr(), stream),
                  "mi_beta_rsample")
    return out


def _launch_categorical(logits: torch.Tensor, strides: Tuple[int, int, int], S: int, T: int,
                        B: int, C: int, seed: int, stream_id: int) -> torch.Tensor:
    """One launch drawing S * T * B categories from logits [S, B, C] read through `strides`."""
    out = torch.empty(S * T * B, dtype=torch.int64, device=logits.device)
    nat.check(nat.lib().mi_predictive_categorical(
        logits.data_ptr(), *strides, S, T, B, C, seed & 0xFFFFFFFFFFFFFFFF, stream_id,
        out.data_ptr(), nat.stream_handle(logits.device)), "mi_predictive_categorical")
    return out


def _draw_batched(family: int, phys: Sequence[torch.Tensor], shape: Tuple[int, ...], seed: int,
                  stream_id: int) -> torch.Tensor:
    """The draw for physical ``[S, ...]`` parameters: ``[S, *shape, *batch]``."""
    S = phys[0].shape[0]
    logical = [tuple(t.shape[1:]) for t in phys]
    batch = tuple(torch.broadcast_shapes(*logical))
    target = (S,) + tuple(shape) + batch
    M = max(1, math.prod(target[1:]))
    params: List[Tuple[torch.Tensor, int, int]] = []
    for t, lg in zip(phys, logical):
        t = t.reshape(S, *([1] * (len(shape) + len(batch) - len(lg))), *lg)
        params.append(_strided(t.expand(target), S, M))
    return _launch(family, params, S, M, seed, stream_id).reshape(target)


class _DrawFn(torch.autograd.Function):
    """draw(index, a, b): one draw per sample; `index` (the sample number, batched under vmap)
    forces the batched rule even when no parameter depends on the sample. One-parameter families
    pass their parameter twice."""
    @staticmethod
    def forward(index, a, b, family, shape, seed, stream_id):  # type: ignore[override]
        # unbatched call (one sample): the sample's own counter block
        out = _draw_batched(family, [a.unsqueeze(0), b.unsqueeze(0)], shape, seed, stream_id)
        return out.squeeze(0)

    @staticmethod
    def setup_context(ctx, inputs, output):  # type: ignore[override]
        ctx.mark_non_differentiable(output)

    @staticmethod
    def vmap(info, in_dims, index, a, b, family, shape, seed, stream_id):  # type: ignore[override]
        S = info.batch_size
        phys = [t.movedim(d, 0) if d is not None else t.expand(S, *t.shape)
                for t, d in zip((a, b), in_dims[1:3])]
        # the samples in the order of `index` (broadcast_particles passes arange(S))
        return _draw_batched(family, phys, shape, seed, stream_id), 0


def _categorical_batched(logits: torch.Tensor, shape: Tuple[int, ...], seed: int,
                         stream_id: int) -> torch.Tensor:
    """Categorical draws for physical logits ``[S, *batch, C]``: ``[S, *shape, *batch]`` int64."""
    S, C = logits.shape[0], logits.shape[-1]
    batch = tuple(logits.shape[1:-1])
    B, T = max(1, math.prod(batch)), max(1, math.prod(shape))
    try:
        rows = logits.view(S, B, C)
    except RuntimeError:
        rows = logits.reshape(S, B, C)
    ss, sb, sc = rows.stride()
    strides = (0 if S == 1 else ss, 0 if B == 1 else sb, 0 if C == 1 else sc)
    out = _launch_categorical(rows, strides, S, T, B, C, seed, stream_id)
    return out.reshape((S,) + tuple(shape) + batch)


class _CategoricalFn(torch.autograd.Function):
    """draw(index, logits): as _DrawFn, for a parameter whose trailing axis is the category axis
    (it stays last and unbroadcast; the batch axes before it are the site's batch_shape)."""
    @staticmethod
    def forward(index, logits, shape, seed, stream_id):  # type: ignore[override]
        return _categorical_batched(logits.unsqueeze(0), shape, seed, stream_id).squeeze(0)

    @staticmethod
    def setup_context(ctx, inputs, output):  # type: ignore[override]
        ctx.mark_non_differentiable(output)

    @staticmethod
    def vmap(info, in_dims, index, logits, shape, seed, stream_id):  # type: ignore[override]
        S = info.batch_size
        d = in_dims[1]
        if d is None:
            phys = logits.expand(S, *logits.shape)
        else:
            # (a batch dimension counted from the end stays clear of the category axis)
            phys = logits.movedim(d if d >= 0 else d + logits.dim(), 0)
        return _categorical_batched(phys, shape, seed, stream_id), 0


def _component_rows(t: torch.Tensor, S: int, B: int, C: int) -> Tuple[torch.Tensor, Tuple]:
    """A physical ``[S, *batch, C]`` parameter as [S, B, C] rows (a view where one exists) and the
    strides to read them through (0 along an axis of one entry or one shared by its entries)."""
    try:
        rows = t.view(S, B, C)
    except RuntimeError:
        rows = t.reshape(S, B, C)
    ss, sb, sc = rows.stride()
    return rows, (0 if S == 1 else ss, 0 if B == 1 else sb, 0 if C == 1 else sc)


def _mixture_batched(phys: Sequence[torch.Tensor], shape: Tuple[int, ...], seed: int,
                     stream_id: int) -> torch.Tensor:
    """Normal-mixture draws for physical logits / loc / scale ``[S, *batch_j, C]`` (each batch_j
    broadcastable to the site's batch shape): ``[S, *shape, *batch]`` float32."""
    S, C = phys[0].shape[0], max(t.shape[-1] for t in phys)
    batch = tuple(torch.broadcast_shapes(*[tuple(t.shape[1:-1]) for t in phys]))
    B, T = max(1, math.prod(batch)), max(1, math.prod(shape))
    args: List = []
    keep = []
    for t in phys:
        t = t.reshape(S, *([1] * (len(batch) - (t.dim() - 2))), *t.shape[1:])
        rows, strides = _component_rows(t.expand(S, *batch, C), S, B, C)
        keep.append(rows)
        args.extend((rows.data_ptr(), *strides))
    device = phys[0].device
    out = torch.empty(S * T * B, dtype=torch.float32, device=device)
    nat.check(nat.lib().mi_predictive_mixture_normal(
        *args, S, T, B, C, seed & 0xFFFFFFFFFFFFFFFF, stream_id, out.data_ptr(),
        nat.stream_handle(device)), "mi_predictive_mixture_normal")
    return out.reshape((S,) + tuple(shape) + batch)


class _MixtureFn(torch.autograd.Function):
    """draw(index, logits, loc, scale): as _CategoricalFn, for three parameters whose trailing
    axis is the component axis."""
    @staticmethod
    def forward(index, logits, loc, scale, shape, seed, stream_id):  # type: ignore[override]
        phys = [t.unsqueeze(0) for t in (logits, loc, scale)]
        return _mixture_batched(phys, shape, seed, stream_id).squeeze(0)

    @staticmethod
    def setup_context(ctx, inputs, output):  # type: ignore[override]
        ctx.mark_non_differentiable(output)

    @staticmethod
    def vmap(info, in_dims, index, logits, loc, scale, shape, seed,
             stream_id):  # type: ignore[override]
        S = info.batch_size
        phys = [t.expand(S, *t.shape) if d is None else
                t.movedim(d if d >= 0 else d + t.dim(), 0)
                for t, d in zip((logits, loc, scale), in_dims[1:4])]
        return _mixture_batched(phys, shape, seed, stream_id), 0


def draw(distribution: Distribution, sample_shape: torch.Size, index: torch.Tensor, seed: int,
         stream_id: int) -> torch.Tensor:
    """``distribution.sample(sample_shape)`` inside the predictive vmap, on the HIP samplers."""
    found = _params(distribution)
    assert found is not None
    family, params = found
    _DRAWS[type(distribution).__name__] += 1
    with torch.no_grad():
        if family == CATEGORICAL:
            logits = params[0].detach()
            if "logits" not in distribution.__dict__:
                logits = torch.log(logits)   # probs: zero stays -inf, never drawn
            return _CategoricalFn.apply(index, logits, tuple(sample_shape), seed,
                                        STREAM_BASE + stream_id)
        if family == MIXTURE_NORMAL:
            logits = params[0].detach()
            if "logits" not in distribution.mixture_distribution.__dict__:
                logits = torch.log(logits)   # probs: zero stays -inf, never drawn
            return _MixtureFn.apply(index, logits, params[1].detach(), params[2].detach(),
                                    tuple(sample_shape), seed, STREAM_BASE + stream_id)
        a, b = params[0].detach(), params[-1].detach()
        return _DrawFn.apply(index, a, b, family, tuple(sample_shape), seed,
                             STREAM_BASE + stream_id)
