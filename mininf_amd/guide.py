"""
Reparameterised guide sampling over K particles (replaces ``FactorizedDistribution.rsample``,
reference ``mininf/nn.py:133-145``, with ONE draw per call at ``nn.py:217``).

Normal, Beta and Gamma factors, and the families of :data:`FAMILIES` (a record each: what the
native sampler accepts, how it is called, its entropy), are drawn by HIP kernels from a
counter-based Philox generator keyed by (seed, step, factor index, global particle index, element),
so that K particles split over W GPUs draw exactly the union of what one GPU would draw. Every
other factor, and one a record's ``accepts`` declines, uses its own ``torch.distributions``
``rsample`` on the device.

Parity mode: ``noise[name]`` injects host-drawn standard normals (Normal factors, [K, *shape];
MultivariateNormal factors, [K, D]; LowRankMultivariateNormal factors, [K, D + R]: eps_D, then
eps_W), the draws themselves (Beta factors) or the standard Gamma
draws g with x = g / rate (Gamma factors) or x = g / sum(g) (Dirichlet factors, [K, *batch, C]),
exactly as the oracle's sample-injection protocol does, or the base noise
[K, *shape] of the one-noise-word families: uniforms in (0, 1), standard normals for HalfNormal
and LogNormal.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
from typing import Callable, Dict, Optional, Tuple

import torch
from torch.distributions import Beta, Cauchy, Dirichlet, Distribution, Exponential, Gamma, \
    HalfCauchy, HalfNormal, Laplace, LogNormal, LowRankMultivariateNormal, MultivariateNormal, Normal

from . import _native as nat
from . import switches


@dataclasses.dataclass
class DrawConfig:
    K: int
    seed: int
    step: int
    stream_id: int
    particle_offset: int
    noise: Optional[torch.Tensor] = None
    step_device: Optional[torch.Tensor] = None   # uint64 word added to `step` on the device
    # The word holding this evaluation's step once the forward has advanced `step_device`
    # (mi_elbo.step_snapshot): read by every kernel that runs after the ELBO forward.
    step_snapshot: Optional[torch.Tensor] = None
    # global index of element 0 (data-sharded factors, mininf_amd.distributed.DataShard)
    element_offset: int = 0
    # the factor is data-sharded (every rank draws its slice), also on the rank whose slice
    # starts at element 0
    sharded: bool = False
    # small Normal factors: leave the launch to the loss's planning (PendingDraw), which may hand
    # the draw to the linear site kernel that reads it (mi_linear.draw)
    defer: bool = False


def backward_step(cfg: DrawConfig) -> Optional[torch.Tensor]:
    """The device step word of a draw's backward (regenerated noise)."""
    return cfg.step_snapshot if cfg.step_snapshot is not None else cfg.step_device


def use_snapshot(cfg: DrawConfig) -> None:
    """Re-evaluate a forward after its ELBO advanced the generator: draw from the snapshot."""
    if cfg.step_snapshot is not None:
        cfg.step_device = cfg.step_snapshot


def _flat_param(t: torch.Tensor, N: int) -> Tuple[torch.Tensor, int]:
    """
    View a parameter of the factor's batch shape as [N] with a single stride (0 for broadcast
    scalars, 1 for contiguous), materialising it otherwise.
    """
    if t.dtype != torch.float32:
        raise nat.NativeError(f"guide parameters must be float32, got {t.dtype}")
    if t.numel() == 1:
        flat = t.reshape(1).expand(N)
        return flat, 0
    flat = t.reshape(N)
    if flat.stride(0) not in (0, 1):
        flat = flat.contiguous()
    return flat, flat.stride(0)


def philox_key(cfg: DrawConfig, backward: bool = False, element: bool = False) -> tuple:
    """
    The Philox key arguments of a native sampler call, in the order of the C ABI: seed, step, the
    device step word (the forward's; with ``backward``, the one its backward regenerates the noise
    from), stream id, particle offset, with ``element`` the element offset (the Normal entry
    points alone take it), injected noise.
    """
    word = backward_step(cfg) if backward else cfg.step_device
    offsets = (cfg.particle_offset, cfg.element_offset) if element else (cfg.particle_offset,)
    return (cfg.seed & 0xFFFFFFFFFFFFFFFF, cfg.step & 0xFFFFFFFFFFFFFFFF, nat.ptr(word),
            cfg.stream_id, *offsets, nat.ptr(cfg.noise))


def _workspace(query: str, *dims: int, device: torch.device) -> Tuple[torch.Tensor, int]:
    """The scratch buffer a sampler's backward asks for through ``query(*dims, &bytes)`` (never
    empty: the library takes its address) and the size asked for."""
    size = ctypes.c_size_t()
    nat.check(getattr(nat.lib(), query)(*dims, ctypes.byref(size)), query)
    return torch.empty(max(1, size.value), dtype=torch.uint8, device=device), size.value


def _float32(grad: torch.Tensor) -> torch.Tensor:
    """An incoming gradient as the float32 the backward kernels read (any strides)."""
    return grad if grad.dtype == torch.float32 else grad.to(torch.float32)


def _inject(cfg: DrawConfig, device: torch.device, *shape: int) -> None:
    """Normalise injected noise, if any, to the contiguous float32 [K, *shape] the samplers read."""
    if cfg.noise is not None:
        cfg.noise = cfg.noise.to(device=device, dtype=torch.float32).reshape(cfg.K, *shape) \
            .contiguous()


# factors each family of FAMILIES drew in the last draw_all, by its counter, and under
# "lowrank_entropy" those whose entropy mi_lowrank_entropy evaluated since (counts())
_DRAWS: "collections.Counter[str]" = collections.Counter()


class _NormalRsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg: DrawConfig, loc: torch.Tensor, loc_s: int, scale: torch.Tensor,
                scale_s: int):  # type: ignore[override]
        N = loc.shape[0]
        K = cfg.K
        z = torch.empty((K, N), dtype=torch.float32, device=loc.device)
        draw = PendingDraw(cfg, z, loc, loc_s, scale, scale_s, exp_source(scale))
        if cfg.defer and cfg.noise is None and (N % 4 == 0 or N == 1) and N <= DEFER_MAX_N and \
                switches.enabled("DRAW_IN_LINEAR"):
            _PENDING_DRAWS[_storage_of(z)] = draw   # launched by flush_draws, or taken
        else:
            draw.launch()
        ctx.cfg = cfg
        ctx.N = N
        ctx.save_for_backward(scale)
        ctx.scale_s = scale_s
        return z

    @staticmethod
    def backward(ctx, dz: torch.Tensor):  # type: ignore[override]
        cfg: DrawConfig = ctx.cfg
        (scale,) = ctx.saved_tensors
        N, K = ctx.N, cfg.K
        device = dz.device
        workspace, size = _workspace("mi_normal_rsample_backward_workspace_bytes", K, N,
                                     device=device)
        dloc = torch.empty(N, dtype=torch.float32, device=device)
        deps_scale = torch.empty(N, dtype=torch.float32, device=device)
        nat.check(nat.lib().mi_normal_rsample_backward(
            dz.data_ptr(), dz.stride(0), dz.stride(1), K, N,
            *philox_key(cfg, backward=True, element=True), workspace.data_ptr(), size,
            dloc.data_ptr(), deps_scale.data_ptr(), nat.stream_handle(device)),
            "mi_normal_rsample_backward")
        # dz/dscale = eps: the kernel returns sum_k dz * eps directly.
        return None, dloc, None, deps_scale, None


def beta_concentration(distribution: Beta, N: int) -> torch.Tensor:
    """
    The [N, 2] (concentration1, concentration0) array torch's Beta keeps for its Dirichlet
    (beta.py:36-40), as one contiguous fp32 tensor: the sampler, its backward and the entropy read
    and write both parameters interleaved, so autograd needs no select/stack kernels.
    """
    dirichlet = getattr(distribution, "_dirichlet", None)
    conc = dirichlet.concentration if dirichlet is not None else \
        torch.stack([distribution.concentration1, distribution.concentration0], -1)
    if conc.dtype != torch.float32:
        raise nat.NativeError(f"guide parameters must be float32, got {conc.dtype}")
    conc = conc.reshape(N, 2)
    return conc if conc.is_contiguous() else conc.contiguous()


# ---- deferred exp transforms of Beta guides ---------------------------------------------------
# ParameterizedDistribution.forward of a Beta guide returns its [.., 2] concentration array
# before anything reads it; the guide's draw (mi_beta_rsample_exp) then computes exp(u) and
# writes the array itself, so the transform needs no launch of its own. Any other reader (torch
# argument validation, .mean, a user's own use) launches the transform first (mi_transform_params).

@dataclasses.dataclass(eq=False)
class _PendingExp:
    out: "weakref.ReferenceType"
    u1: torch.Tensor
    u0: Optional[torch.Tensor]   # None: a single positive parameter (a Normal guide's scale)
    params: object          # the mi_params of the transform launch
    filled: bool = False


_PENDING_EXP: Dict[int, _PendingExp] = {}


def _storage_of(tensor) -> Optional[int]:
    if not isinstance(tensor, torch.Tensor):
        return None
    try:
        return tensor.untyped_storage().data_ptr()
    except (RuntimeError, NotImplementedError):
        return None


def pending_exp(tensor) -> Optional[_PendingExp]:
    """The pending transform a concentration array (or a view of it) waits for, or None."""
    if not _PENDING_EXP:
        return None
    rec = _PENDING_EXP.get(_storage_of(tensor))
    if rec is None or rec.filled or rec.out() is None:
        return None
    return rec


def exp_source(scale) -> Optional[Tuple[_PendingExp, int]]:
    """
    For a Normal guide scale still waiting for its exp transform: the record and the address of
    the unconstrained parameter element that becomes ``scale``'s first element, so a kernel can
    read exp(u) at ``scale``'s own offset and strides and write it (mi_normal_rsample_exp,
    mi_draw.scale_exp). None when nothing is pending or the layouts differ.
    """
    rec = pending_exp(scale)
    out = rec.out() if rec is not None else None
    if out is None or rec.u0 is not None or not rec.u1.is_contiguous() or \
            not out.is_contiguous() or tuple(rec.u1.shape) != tuple(out.shape):
        return None
    # u has the layout of the (contiguous) transform output: same offset, same strides
    return rec, rec.u1.data_ptr() + (scale.data_ptr() - out.data_ptr())


def fill_exp(tensor) -> None:
    """Launch a pending transform (mi_transform_params) before its array is read."""
    rec = pending_exp(tensor)
    if rec is None:
        return
    out = rec.out()
    nat.check(nat.lib().mi_transform_params(ctypes.byref(rec.params), out.data_ptr(),
                                            nat.stream_handle(out.device)), "mi_transform_params")
    rec.filled = True


def _forget_exp(ptr: int, rec: _PendingExp) -> None:
    if _PENDING_EXP.get(ptr) is rec:
        del _PENDING_EXP[ptr]


def defer_exp(out: torch.Tensor, u1: torch.Tensor, u0: Optional[torch.Tensor],
              params) -> torch.Tensor:
    """Register `out` (a PendingConcentration) as the pending exp-stack of (u1, u0). The record
    lives as long as `out` does; views of it keep `out` alive."""
    import weakref
    ptr = _storage_of(out)
    rec = _PendingExp(weakref.ref(out), u1, u0, params)
    _PENDING_EXP[ptr] = rec
    weakref.finalize(out, _forget_exp, ptr, rec)
    return out


_PENDING_METADATA = {
    torch.Tensor.size, torch.Tensor.dim, torch.Tensor.ndimension, torch.Tensor.numel,
    torch.Tensor.__len__, torch.Tensor.is_floating_point, torch.Tensor.stride,
    torch.Tensor.element_size, torch.Tensor.data_ptr, torch.Tensor.untyped_storage,
    torch.Tensor.storage_offset, torch.Tensor.is_contiguous, torch.Tensor.shape.__get__,
    torch.Tensor.dtype.__get__, torch.Tensor.device.__get__, torch.Tensor.ndim.__get__,
    torch.Tensor.requires_grad.__get__, torch.Tensor.is_cuda.__get__, torch.Tensor.layout.__get__,
    torch.Tensor.grad_fn.__get__, torch.Tensor.is_leaf.__get__, torch.Tensor.__hash__,
    torch.Tensor._version.__get__, torch.Tensor.reshape, torch.Tensor.view,
}


# views (no value read): the results stay pending
_PENDING_VIEWS = {torch.Tensor.reshape, torch.Tensor.view, torch.Tensor.expand,
                  torch.Tensor.expand_as, torch.broadcast_to, torch.Tensor.broadcast_to,
                  torch.broadcast_tensors, torch.functional.broadcast_tensors}


class PendingConcentration(torch.Tensor):
    """A guide parameter array whose exp transform has not run yet (a Beta guide's concentrations,
    a Normal guide's scale; see above): shape queries, views and pointer reads pass through;
    anything else launches the transform first."""
    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        copies = func is torch.Tensor.reshape and args and isinstance(args[0], torch.Tensor) and \
            not args[0].is_contiguous()   # a reshape that copies reads the values
        if (func not in _PENDING_METADATA and func not in _PENDING_VIEWS) or copies:
            stack = [args, kwargs]
            while stack:
                x = stack.pop()
                if isinstance(x, PendingConcentration):
                    fill_exp(x)
                elif isinstance(x, (list, tuple)):
                    stack.extend(x)
                elif isinstance(x, dict):
                    stack.extend(x.values())
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **kwargs)
        if func in _PENDING_VIEWS:
            roots = [x for x in _flat_args(args) if isinstance(x, PendingConcentration)]

            def rewrap(t):
                if isinstance(t, torch.Tensor) and pending_exp(t) is not None:
                    t = t.as_subclass(PendingConcentration)
                    t._pending_root = roots   # keeps the pending records' tensors alive
                return t
            if isinstance(out, (tuple, list)):
                out = type(out)(rewrap(t) for t in out)
            else:
                out = rewrap(out)
        return out


def _flat_args(args):
    stack, flat = [args], []
    while stack:
        x = stack.pop()
        if isinstance(x, (list, tuple)):
            stack.extend(x)
        else:
            flat.append(x)
    return flat


class _BetaRsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg: DrawConfig, conc: torch.Tensor):  # type: ignore[override]
        N = conc.shape[0]
        K = cfg.K
        x = torch.empty((K, N), dtype=torch.float32, device=conc.device)
        base = conc.data_ptr()
        pending = pending_exp(conc)
        if pending is not None:   # the guide's exp transform and the draw in one launch
            u1, u0 = pending.u1.reshape(-1), pending.u0.reshape(-1)
            nat.check(nat.lib().mi_beta_rsample_exp(
                u1.data_ptr(), u1.stride(0) if u1.numel() > 1 else 0, u0.data_ptr(),
                u0.stride(0) if u0.numel() > 1 else 0, base, K, N, *philox_key(cfg),
                x.data_ptr(), nat.stream_handle(conc.device)), "mi_beta_rsample_exp")
            pending.filled = True
        else:
            nat.check(nat.lib().mi_beta_rsample(
                base, 2, base + 4, 2, K, N, *philox_key(cfg), x.data_ptr(),
                nat.stream_handle(conc.device)), "mi_beta_rsample")
        ctx.save_for_backward(x, conc)
        ctx.K, ctx.N = K, N
        return x

    @staticmethod
    def backward(ctx, dx: torch.Tensor):  # type: ignore[override]
        x, conc = ctx.saved_tensors
        K, N = ctx.K, ctx.N
        device = dx.device
        workspace, size = _workspace("mi_beta_rsample_backward_workspace_bytes", K, N,
                                     device=device)
        dconc = torch.empty((N, 2), dtype=torch.float32, device=device)
        base, out = conc.data_ptr(), dconc.data_ptr()
        nat.check(nat.lib().mi_beta_rsample_backward(
            dx.data_ptr(), dx.stride(0), dx.stride(1), x.data_ptr(), base, 2, base + 4, 2, K, N,
            workspace.data_ptr(), size, out, 2, out + 4, 2, nat.stream_handle(device)),
            "mi_beta_rsample_backward")
        return None, dconc


def gamma_params(distribution: Gamma, N: int) -> Tuple[torch.Tensor, int, torch.Tensor, int]:
    """(concentration, stride, rate, stride) of a Gamma factor viewed as [N]."""
    conc, conc_s = _flat_param(distribution.concentration, N)
    rate, rate_s = _flat_param(distribution.rate, N)
    return conc, conc_s, rate, rate_s


@dataclasses.dataclass(frozen=True)
class _Sampler:
    """
    How :class:`_RsampleFn` calls one family's entry points ``<stem>``, ``<stem>_backward`` and
    ``<stem>_backward_workspace_bytes``. With ``inputs`` the family's arguments of
    ``_RsampleFn.apply`` (tensors go by address), the forward is
    ``<stem>(*inputs, K, *sizes, *key, [g,] out, stream)`` and the backward
    ``<stem>_backward(*reads, K, *sizes, [*key,] workspace, bytes, *gradients, stream)``.
    """
    stem: str
    # positions among the inputs of the float32 parameters: one gradient each, of the parameter's
    # shape; the first has the shape of one particle's draw
    params: Tuple[int, ...]
    saves: Tuple[int, ...]   # positions of the inputs the backward reads
    sizes: Callable          # (*inputs) -> the sizes that follow K in the three entry points
    # (dz and its strides, the inputs with only the saved tensors' addresses, the saved draws'
    # address) -> the backward's arguments before K
    reads: Callable
    # The backward of a family without saved draws regenerates the noise from the key. "out": it
    # reads the draws instead; "standard": the standard draws g, which the forward writes as well.
    draws: Optional[str] = None
    after_gradient: Tuple[int, ...] = ()   # follows every gradient address (Gamma: its stride)
    # a gradient nobody needs is null, and nothing is launched when none is needed; the other
    # families always write all of theirs
    optional: bool = False


class _RsampleFn(torch.autograd.Function):
    """K reparameterised draws of one guide factor through its family's :class:`_Sampler`."""
    @staticmethod
    def forward(ctx, family: _Sampler, cfg: DrawConfig, *inputs):  # type: ignore[override]
        K, first = cfg.K, inputs[family.params[0]]
        sizes = tuple(family.sizes(*inputs))
        out = torch.empty((K,) + tuple(first.shape), dtype=torch.float32, device=first.device)
        g = torch.empty_like(out) if family.draws == "standard" else None
        nat.check(getattr(nat.lib(), family.stem)(
            *(nat.ptr(x) if isinstance(x, torch.Tensor) else x for x in inputs), K, *sizes,
            *philox_key(cfg), *(() if g is None else (g.data_ptr(),)), out.data_ptr(),
            nat.stream_handle(first.device)), family.stem)
        ctx.family, ctx.cfg, ctx.sizes = family, cfg, sizes
        ctx.shapes = [tuple(inputs[i].shape) if inputs[i] is not None else None
                      for i in family.params]
        ctx.args = [None if isinstance(x, torch.Tensor) else x for x in inputs]
        ctx.save_for_backward(*(inputs[i] for i in family.saves),
                              *((g,) if g is not None else (out,) if family.draws else ()))
        return out

    @staticmethod
    def backward(ctx, dz: torch.Tensor):  # type: ignore[override]
        family, cfg, K = ctx.family, ctx.cfg, ctx.cfg.K
        grads = [None] * (2 + len(ctx.args))
        need = [shape is not None and (not family.optional or ctx.needs_input_grad[2 + i])
                for i, shape in zip(family.params, ctx.shapes)]
        if not any(need):
            return tuple(grads)
        device, dz = dz.device, _float32(dz)
        inputs, saved = list(ctx.args), ctx.saved_tensors
        for i, tensor in zip(family.saves, saved):
            inputs[i] = nat.ptr(tensor)
        workspace, size = _workspace(family.stem + "_backward_workspace_bytes", K, *ctx.sizes,
                                     device=device)
        pointers = []
        for i, shape, wanted in zip(family.params, ctx.shapes, need):
            if wanted:
                grads[2 + i] = torch.empty(shape, dtype=torch.float32, device=device)
            pointers += [nat.ptr(grads[2 + i]), *family.after_gradient]
        nat.check(getattr(nat.lib(), family.stem + "_backward")(
            *family.reads((dz.data_ptr(), *dz.stride()), inputs,
                          saved[-1].data_ptr() if family.draws else None), K, *ctx.sizes,
            *(() if family.draws else philox_key(cfg, backward=True)), workspace.data_ptr(), size,
            *pointers, nat.stream_handle(device)), family.stem + "_backward")
        # (per element: a broadcast parameter's expand backward sums them)
        return tuple(grads)


# Gamma.rsample (gamma.py:80-88): inputs (concentration, stride, rate, stride), as gamma_params
# gives them. The backward is torch._standard_gamma_grad restated in fp64. ``cfg.noise`` injects
# the standard Gamma draws g (x = g / rate), the oracle's protocol for Gamma factors.
_GAMMA = _Sampler("mi_gamma_rsample", params=(0, 2), saves=(0, 2), draws="standard",
                  after_gradient=(1,), sizes=lambda conc, *_: conc.shape,
                  reads=lambda dx, inputs, g: (*dx, g, *inputs))
# MultivariateNormal.rsample (multivariate_normal.py:247-250): inputs (loc [D], scale_tril [D, D]);
# z = loc + eps @ scale_tril^T with the Philox eps of a Normal factor of D elements. ``cfg.noise``
# injects eps [K, D], as for a Normal factor.
_MVN = _Sampler("mi_mvn_rsample", params=(0, 1), saves=(), sizes=lambda loc, tril: loc.shape,
                reads=lambda dz, inputs, _: dz)
# LowRankMultivariateNormal.rsample (lowrank_multivariate_normal.py:214-223): inputs (loc [D],
# cov_factor [D, R], cov_diag [D]); z = loc + eps_W @ cov_factor^T + sqrt(cov_diag) * eps_D, both
# sets of normals from the factor's one Normal stream (eps_D: elements [0, D); eps_W: elements
# [Dpad, Dpad + R)). ``cfg.noise`` injects [K, D + R]: eps_D, then eps_W.
_LOWRANK = _Sampler("mi_lowrank_rsample", params=(0, 1, 2), saves=(2,),
                    sizes=lambda loc, cov_factor, cov_diag: cov_factor.shape,
                    reads=lambda dz, inputs, _: (*dz, inputs[2]))
# Dirichlet.rsample (dirichlet.py:85-88): input (concentration [N, C]); normalised standard Gamma
# draws, and _Dirichlet_backward (dirichlet.py:17-20) in fp64 from the saved draws. ``cfg.noise``
# injects the standard Gamma draws g [K, N, C], as for a Gamma factor.
_DIRICHLET = _Sampler("mi_dirichlet_rsample", params=(0,), saves=(0,), draws="out",
                      sizes=lambda conc: conc.shape,
                      reads=lambda dx, inputs, x: (*dx, x, *inputs))
# The one-noise-word families: inputs (MI_PRED_* code, a [N], stride, b [N] or None, stride), as
# _elementwise_params gives them. ``cfg.noise`` injects the base noise [K, N]: uniforms, or
# standard normals for HalfNormal and LogNormal.
_ELEMENTWISE_SAMPLER = _Sampler("mi_elementwise_rsample", params=(1, 3), saves=(1, 3),
                                optional=True, sizes=lambda code, a, *_: a.shape,
                                reads=lambda dz, inputs, _: (inputs[0], *dz, *inputs[1:]))


class _EntropyFn(torch.autograd.Function):
    """
    A factor's summed entropy and its gradients in one launch: ``launch(needs, *inputs)`` (``needs``
    this node's needs_input_grad of the inputs) returns the 0-d value and one gradient per input,
    None where there is none. The backward scales the stored gradients.
    """
    @staticmethod
    def forward(ctx, launch: Callable, *inputs):  # type: ignore[override]
        out, ctx.grads = launch(ctx.needs_input_grad[1:], *inputs)
        return out

    @staticmethod
    def backward(ctx, g: torch.Tensor):  # type: ignore[override]
        return (None, *(None if grad is None else grad * g for grad in ctx.grads))


def native_mvn(distribution) -> bool:
    """
    Whether a MultivariateNormal guide factor is drawn by mi_mvn_rsample (and its entropy evaluated
    by the ELBO kernels): unbatched, float32, on the device, D <= MI_MVN_MAX_N. Any other
    MultivariateNormal keeps torch's own rsample and entropy.
    """
    if type(distribution) is not MultivariateNormal or tuple(distribution.batch_shape) != ():
        return False
    loc = distribution.loc
    return loc.is_cuda and loc.dtype == torch.float32 and \
        1 <= int(distribution.event_shape[0]) <= nat.MVN_MAX_N


def _mvn_inputs(distribution: MultivariateNormal):
    """(:data:`_MVN`'s inputs, the shape of the injected noise after K, that of the result) of a
    :func:`native_mvn` factor."""
    # the public properties: scale_tril carries the autograd of a covariance_matrix /
    # precision_matrix parameterisation
    D = int(distribution.event_shape[0])
    loc = distribution.loc.reshape(D).contiguous()
    scale_tril = distribution.scale_tril.reshape(D, D)
    if scale_tril.dtype != torch.float32:
        raise nat.NativeError(f"guide parameters must be float32, got {scale_tril.dtype}")
    return (loc, scale_tril.contiguous()), (D,), (D,)   # eps, [K, D]


def native_lowrank(distribution) -> bool:
    """
    Whether a LowRankMultivariateNormal guide factor is drawn by mi_lowrank_rsample (and its
    entropy evaluated by mi_lowrank_entropy): exactly that class (a subclass may override rsample
    or entropy), unbatched, float32, on the device, R <= MI_LOWRANK_MAX_R and
    D <= MI_LOWRANK_MAX_D. Any other keeps torch's own rsample and entropy.
    """
    if type(distribution) is not LowRankMultivariateNormal or \
            tuple(distribution.batch_shape) != ():
        return False
    loc = distribution.loc
    W, diag = distribution._unbroadcasted_cov_factor, distribution._unbroadcasted_cov_diag
    return loc.is_cuda and all(t.dtype == torch.float32 for t in (loc, W, diag)) and \
        W.dim() == 2 and diag.dim() == 1 and \
        1 <= int(W.shape[-1]) <= nat.LOWRANK_MAX_R and \
        1 <= int(distribution.event_shape[0]) <= nat.LOWRANK_MAX_D


def _lowrank_inputs(distribution: LowRankMultivariateNormal):
    """(:data:`_LOWRANK`'s inputs, the shape of the injected noise after K, that of the result) of
    a :func:`native_lowrank` factor."""
    # the public loc and the unbroadcast cov_factor / cov_diag (of an unbatched factor: the
    # constructor's own arguments, which carry the autograd of the parameterisation)
    cov_factor = distribution._unbroadcasted_cov_factor
    cov_diag = distribution._unbroadcasted_cov_diag
    fill_exp(cov_diag)
    D, R = (int(n) for n in cov_factor.shape)
    loc = distribution.loc.reshape(D).contiguous()
    # eps_D | eps_W, [K, D + R]
    return (loc, cov_factor.contiguous(), cov_diag.contiguous()), (D + R,), (D,)


def _lowrank_entropy(needs, cov_factor: torch.Tensor, cov_diag: torch.Tensor, tril: torch.Tensor):
    """
    LowRankMultivariateNormal.entropy() (lowrank_multivariate_normal.py:225-237) and its gradient
    with respect to cov_factor and cov_diag in closed form, in one mi_lowrank_entropy call.
    ``tril`` is the factor's _capacitance_tril, detached: the closed form carries its whole
    dependence on the two parameters.
    """
    D, R = cov_factor.shape
    device = cov_factor.device
    out = torch.empty((), dtype=torch.float32, device=device)
    grads = cov_factor.requires_grad or cov_diag.requires_grad
    dfactor = torch.empty_like(cov_factor) if grads else None
    ddiag = torch.empty_like(cov_diag) if grads else None
    workspace, size = _workspace("mi_lowrank_entropy_workspace_bytes", D, R, device=device)
    nat.check(nat.lib().mi_lowrank_entropy(
        cov_factor.data_ptr(), cov_diag.data_ptr(), tril.data_ptr(), D, R,
        workspace.data_ptr(), size, out.data_ptr(), nat.ptr(dfactor), nat.ptr(ddiag),
        nat.stream_handle(device)), "mi_lowrank_entropy")
    return out, (dfactor, ddiag, None)


def lowrank_entropy(distribution: LowRankMultivariateNormal) -> torch.Tensor:
    """The entropy of a :func:`native_lowrank` guide factor (0-d, differentiable with respect to
    cov_factor and cov_diag; nothing flows into the constructor's capacitance graph)."""
    cov_factor = distribution._unbroadcasted_cov_factor
    cov_diag = distribution._unbroadcasted_cov_diag
    fill_exp(cov_diag)
    tril = distribution._capacitance_tril.detach()
    _DRAWS["lowrank_entropy"] += 1
    return _EntropyFn.apply(_lowrank_entropy, cov_factor.contiguous(), cov_diag.contiguous(),
                            tril.contiguous())


def native_dirichlet(distribution) -> bool:
    """
    Whether a Dirichlet guide factor is drawn by mi_dirichlet_rsample (and its entropy evaluated by
    mi_dirichlet_entropy): exactly a Dirichlet (a subclass may override rsample), float32, on the
    device, C <= MI_DIRICHLET_MAX_C. Any other Dirichlet keeps torch's own rsample and entropy.
    """
    if type(distribution) is not Dirichlet:
        return False
    conc = distribution.concentration
    return isinstance(conc, torch.Tensor) and conc.is_cuda and conc.dtype == torch.float32 and \
        1 <= int(conc.shape[-1]) <= nat.DIRICHLET_MAX_C


def _dirichlet_rows(distribution: Dirichlet) -> torch.Tensor:
    """The concentration as a contiguous [N, C] array (N = numel(batch_shape))."""
    conc = distribution.concentration
    fill_exp(conc)
    C = int(conc.shape[-1])
    return conc.reshape(max(1, int(distribution.batch_shape.numel())), C).contiguous()


def _dirichlet_inputs(distribution: Dirichlet):
    """(:data:`_DIRICHLET`'s input, the shape of the injected noise after K, that of the result) of
    a :func:`native_dirichlet` factor."""
    conc = _dirichlet_rows(distribution)
    # standard draws g, [K, *batch, C]
    return (conc,), tuple(conc.shape), tuple(distribution.batch_shape) + (int(conc.shape[1]),)


def _dirichlet_entropy(needs, conc: torch.Tensor):
    """Dirichlet.entropy().sum() (dirichlet.py:122-130) and its gradient in one launch
    (mi_dirichlet_entropy)."""
    N, C = conc.shape
    out = torch.empty((), dtype=torch.float32, device=conc.device)
    grad = torch.empty_like(conc) if conc.requires_grad else None
    nat.check(nat.lib().mi_dirichlet_entropy(
        conc.data_ptr(), N, C, out.data_ptr(), nat.ptr(grad),
        nat.stream_handle(conc.device)), "mi_dirichlet_entropy")
    return out, (grad,)


def dirichlet_entropy(distribution: Dirichlet) -> torch.Tensor:
    """The summed entropy of a :func:`native_dirichlet` guide factor (0-d, differentiable)."""
    return _EntropyFn.apply(_dirichlet_entropy, _dirichlet_rows(distribution))


# ---- one-noise-word families -------------------------------------------------------------------
# class -> MI_PRED_* code of mi_elementwise_rsample
_ELEMENTWISE = {Exponential: nat.PRED_EXPONENTIAL, Laplace: nat.PRED_LAPLACE,
                Cauchy: nat.PRED_CAUCHY, HalfCauchy: nat.PRED_HALF_CAUCHY,
                HalfNormal: nat.PRED_HALF_NORMAL, LogNormal: nat.PRED_LOG_NORMAL}


def _elementwise_arguments(distribution) -> Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """The (a, b) parameters of mi_elementwise_rsample's table as the distribution holds them
    (LogNormal and the half families: inside ``base_dist``), or None when they are not there."""
    cls = type(distribution)
    if cls is Exponential:
        params = (getattr(distribution, "rate", None), None)
    elif cls is Laplace or cls is Cauchy:
        params = (getattr(distribution, "loc", None), getattr(distribution, "scale", None))
    else:
        base = getattr(distribution, "base_dist", None)
        if type(base) is not (Cauchy if cls is HalfCauchy else Normal):
            return None
        params = (base.loc, base.scale) if cls is LogNormal else (base.scale, None)
    if not isinstance(params[0], torch.Tensor) or \
            not (params[1] is None or isinstance(params[1], torch.Tensor)):
        return None
    return params


def native_elementwise(distribution) -> bool:
    """
    Whether a guide factor is drawn by mi_elementwise_rsample (and its entropy evaluated by
    mi_elementwise_entropy): exactly an Exponential, Laplace, Cauchy, HalfCauchy, HalfNormal or
    LogNormal (a subclass may override rsample; a TransformedDistribution spelled out by hand has
    no entropy), float32, on the device. Any other keeps torch's own rsample and entropy.
    """
    if type(distribution) not in _ELEMENTWISE:
        return False
    params = _elementwise_arguments(distribution)
    return params is not None and all(t is None or (t.is_cuda and t.dtype == torch.float32)
                                      for t in params)


def _elementwise_params(distribution, N: int):
    """(family, a, a stride, b or None, b stride) of a :func:`native_elementwise` factor viewed
    as [N]; a deferred exp transform of a positive parameter runs first."""
    a, b = _elementwise_arguments(distribution)
    fill_exp(a)
    a, a_s = _flat_param(a, N)
    b_s = 0
    if b is not None:
        fill_exp(b)
        b, b_s = _flat_param(b, N)
    return _ELEMENTWISE[type(distribution)], a, a_s, b, b_s


def _elementwise_inputs(distribution):
    """(:data:`_ELEMENTWISE_SAMPLER`'s inputs, the shape of the injected noise after K, that of the
    result) of a :func:`native_elementwise` factor."""
    shape = tuple(distribution.batch_shape)
    N = max(1, int(distribution.batch_shape.numel()))
    # base noise (uniforms or normals), [K, *shape]
    return _elementwise_params(distribution, N), (N,), shape


def _elementwise_entropy(needs, family: int, a: torch.Tensor, a_s: int,
                         b: Optional[torch.Tensor], b_s: int):
    """entropy().sum() of a one-noise-word factor and its gradient in one launch
    (mi_elementwise_entropy)."""
    N = a.shape[0]
    out = torch.empty((), dtype=torch.float32, device=a.device)
    # (the entropy of a Laplace or Cauchy factor does not depend on its loc)
    da = torch.empty(N, dtype=torch.float32, device=a.device) if needs[1] and \
        family not in (nat.PRED_LAPLACE, nat.PRED_CAUCHY) else None
    db = torch.empty(N, dtype=torch.float32, device=a.device) if b is not None and \
        needs[3] else None
    nat.check(nat.lib().mi_elementwise_entropy(
        family, a.data_ptr(), a_s, nat.ptr(b), b_s, N, out.data_ptr(), nat.ptr(da),
        nat.ptr(db), nat.stream_handle(a.device)), "mi_elementwise_entropy")
    return out, (None, da, None, db, None)


def elementwise_entropy(distribution) -> torch.Tensor:
    """The summed entropy of a :func:`native_elementwise` guide factor (0-d, differentiable)."""
    N = max(1, int(distribution.batch_shape.numel()))
    return _EntropyFn.apply(_elementwise_entropy, *_elementwise_params(distribution, N))


# ---- the family table --------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Family:
    """A family of guide factors beyond Normal, Beta and Gamma with a native sampler."""
    counter: str        # the key in _DRAWS; counts()["<counter>_draws"]
    accepts: Callable   # (distribution) -> whether the native sampler draws it
    sampler: _Sampler
    # (distribution) -> (the sampler's inputs, the shape after K of the noise injected, that of
    # the result)
    prepare: Callable
    # (distribution) -> its summed entropy by the family's own kernel; None: the ELBO kernels
    # evaluate it (engine.entropy_factors), or else torch
    entropy: Optional[Callable]


# read by draw(), entropy() and counts()
FAMILIES: Tuple[Family, ...] = (
    Family("mvn", native_mvn, _MVN, _mvn_inputs, None),
    Family("dirichlet", native_dirichlet, _DIRICHLET, _dirichlet_inputs, dirichlet_entropy),
    Family("lowrank", native_lowrank, _LOWRANK, _lowrank_inputs, lowrank_entropy),
    Family("elementwise", native_elementwise, _ELEMENTWISE_SAMPLER, _elementwise_inputs,
           elementwise_entropy),
)


def entropy(factor: Distribution) -> torch.Tensor:
    """The summed entropy of a guide factor the ELBO kernels do not evaluate
    (engine.entropy_factors' rest): by the family's own kernel where it has one, else torch's."""
    for family in FAMILIES:
        if family.entropy is not None and family.accepts(factor):
            return family.entropy(factor)
    return factor.entropy().sum()


def counts() -> Dict[str, int]:
    """Factors each family's native sampler drew in the last draw_all, and LowRankMultivariateNormal
    factors whose entropy mi_lowrank_entropy evaluated since
    (EvidenceLowerBoundLoss.last_fusions merges them)."""
    return {**{family.counter + "_draws": _DRAWS[family.counter] for family in FAMILIES},
            "lowrank_entropies": _DRAWS["lowrank_entropy"]}


# ---- deferred small Normal draws ---------------------------------------------------------------
# A small Normal factor's [K, N] draw (the regression's theta, N = P features) is made by the loss's
# planning instead of when the guide is drawn: when the only kernel that reads it is one linear
# site, that launch draws it (mi_linear.draw, one launch less per step); otherwise flush_draws
# launches mi_normal_rsample before anything reads it (the particle trace's torch operations flush
# through mininf_amd.linear.DeferredMatmul).
DEFER_MAX_N = 64   # MI_LINEAR_MAX_P

@dataclasses.dataclass(eq=False)
class PendingDraw:
    cfg: DrawConfig
    z: torch.Tensor
    loc: torch.Tensor
    loc_s: int
    scale: torch.Tensor
    scale_s: int
    source: Optional[Tuple["_PendingExp", int]]   # exp_source(scale) at draw time
    done: bool = False
    claimed: bool = False   # a planned linear launch will make it (engine.claim_linear_draws)

    def launch(self) -> None:
        """mi_normal_rsample (or _exp with the guide's pending exp transform) into z."""
        if self.done:
            return
        self.done = True
        cfg, loc, scale, z = self.cfg, self.loc, self.scale, self.z
        K, N = z.shape
        if self.source is not None:
            # the guide's exp transform and the draw in one launch
            pending, u_ptr = self.source
            nat.check(nat.lib().mi_normal_rsample_exp(
                loc.data_ptr(), self.loc_s, u_ptr, self.scale_s, scale.data_ptr(), K, N,
                *philox_key(cfg, element=True), z.data_ptr(), nat.stream_handle(loc.device)),
                "mi_normal_rsample_exp")
            pending.filled = True
        else:
            fill_exp(scale)
            nat.check(nat.lib().mi_normal_rsample(
                loc.data_ptr(), self.loc_s, scale.data_ptr(), self.scale_s, K, N,
                *philox_key(cfg, element=True), z.data_ptr(), nat.stream_handle(loc.device)),
                "mi_normal_rsample")

    def describe(self, D) -> None:
        """Fill an mi_draw descriptor for the linear site kernel that takes this draw over."""
        D.operand = 1
        D.loc, D.loc_stride = self.loc.data_ptr(), self.loc_s
        D.scale, D.scale_stride = self.scale.data_ptr(), self.scale_s
        D.scale_exp = self.source[1] if self.source is not None else None
        # (a deferred draw has no injected noise)
        D.seed, D.step, D.step_device, D.stream_id, D.particle_offset, D.element_offset, _ = \
            philox_key(self.cfg, element=True)

    def taken(self) -> None:
        """The linear launch made the draw (and the pending exp transform of its scale)."""
        self.done = True
        if self.source is not None:
            self.source[0].filled = True


_PENDING_DRAWS: Dict[Optional[int], PendingDraw] = {}


def pending_draw(tensor) -> Optional[PendingDraw]:
    """The not yet launched draw whose storage `tensor` (or a batched view of it) reads, or None."""
    if not _PENDING_DRAWS or not isinstance(tensor, torch.Tensor):
        return None
    functorch = torch._C._functorch
    base = tensor
    while functorch.is_batchedtensor(base):
        base = functorch.get_unwrapped(base)
    rec = _PENDING_DRAWS.get(_storage_of(base))
    return rec if rec is not None and not rec.done else None


def flush_draws(claimed: bool = False) -> None:
    """Launch every deferred draw no linear launch has claimed (with ``claimed``, those too)
    before anything reads them."""
    for key, rec in list(_PENDING_DRAWS.items()):
        if claimed or not rec.claimed:
            del _PENDING_DRAWS[key]
            rec.launch()


def take_draw(rec: PendingDraw) -> None:
    rec.taken()
    _PENDING_DRAWS.pop(_storage_of(rec.z), None)


@dataclasses.dataclass(eq=False)   # identity semantics: used in sets
class LazyDraw:
    r"""
    A Normal factor's K draws left to the site kernels (``mi_draw``): the model is traced with
    ``placeholder`` -- a [K, *shape] zero-stride view of a private one-element buffer, recognised
    by its data pointer -- and site groups that read it compute ``loc + eps * scale`` in registers
    (the same Philox eps as :class:`_NormalRsampleFn`). Any other use of the draw in the model
    makes the loss re-trace with :meth:`materialize`\ d draws.
    """
    cfg: DrawConfig
    loc: torch.Tensor
    loc_s: int
    scale: torch.Tensor
    scale_s: int
    N: int
    shape: torch.Size
    placeholder: torch.Tensor
    real: Optional[torch.Tensor] = None

    def materialize(self) -> torch.Tensor:
        if self.real is None:
            z = _NormalRsampleFn.apply(self.cfg, self.loc, self.loc_s, self.scale, self.scale_s)
            self.real = z.reshape((self.cfg.K,) + tuple(self.shape))
            _DRAWN[self.real.data_ptr()] = Drawn(NORMAL_FAMILY, self.cfg, z, self.N)
        return self.real


# data pointer of a live placeholder -> its draw (reset by every lazy draw_all)
_LAZY: Dict[int, LazyDraw] = {}

NORMAL_FAMILY, BETA_FAMILY = "normal", "beta"


@dataclasses.dataclass(eq=False)
class Drawn:
    """
    A materialised guide draw of the last draw_all: ``base`` is the [K, N] output of the sampler's
    autograd node (Normal: :class:`_NormalRsampleFn`, Beta: :class:`_BetaRsampleFn`), from which
    the ELBO can take over the draw's backward (``mi_factor`` absorbed draws).
    """
    family: str
    cfg: DrawConfig
    base: torch.Tensor
    N: int
    dgrad: Optional[torch.Tensor] = None   # Beta: mi_beta_dgrad factors [K, N, 2] (side stream)
    conc: Optional[torch.Tensor] = None    # Beta: the interleaved [N, 2] concentration drawn from


# data pointer of a materialised draw -> its record (reset by every draw_all)
_DRAWN: Dict[int, Drawn] = {}

# Work launched on a side stream by the draws (Beta implicit-gradient factors) that the main
# stream has not joined yet: joined by join_side() before the ELBO reads it, and always before a
# captured step ends.
_SIDE_STREAMS: Dict[int, torch.cuda.Stream] = {}
_PENDING: list = []
# fp64 [K, N, 2] factors up to this many draws (64 MiB); larger Beta factors are evaluated inside
# mi_elbo_forward as before
BETA_DGRAD_MAX = 1 << 22


def _side_stream(device: torch.device) -> torch.cuda.Stream:
    index = device.index if device.index is not None else torch.cuda.current_device()
    stream = _SIDE_STREAMS.get(index)
    if stream is None:
        stream = _SIDE_STREAMS[index] = torch.cuda.Stream(device=device)
    return stream


def join_side() -> None:
    """Make the current stream wait for the side-stream work of the last draws."""
    if not _PENDING:
        return
    current = torch.cuda.current_stream()
    for event in _PENDING:
        current.wait_event(event)
    _PENDING.clear()


def _beta_dgrad(x: torch.Tensor, conc: torch.Tensor, K: int, N: int) -> Optional[torch.Tensor]:
    """
    Launch mi_beta_dgrad for the draws x on the side stream (MININF_AMD_BETA_DGRAD=1): its fp64
    chains depend only on the draws, so they can run beside the site kernels instead of inside
    mi_elbo_forward. Off by default: measured on MI355X (C2, hipGraph replay) the two-queue graph
    cost more per node than the overlap saved (0.17 -> 0.24 ms per step).
    """
    if not (torch.is_grad_enabled() and conc.requires_grad) or K * N > BETA_DGRAD_MAX or \
            not switches.enabled("BETA_DGRAD", default=False):
        return None
    main = torch.cuda.current_stream()
    side = _side_stream(x.device)
    out = torch.empty((K, N, 2), dtype=torch.float64, device=x.device)
    side.wait_stream(main)
    base = conc.data_ptr()
    nat.check(nat.lib().mi_beta_dgrad(x.data_ptr(), base, 2, base + 4, 2, K, N, out.data_ptr(),
                                      side.cuda_stream), "mi_beta_dgrad")
    event = torch.cuda.Event()
    event.record(side)
    # main-stream tensors used on the side stream: not reused before the side work is done
    for t in (x, conc, out):
        t.record_stream(side)
    _PENDING.append(event)
    return out


def release_lazy() -> None:
    """
    Forget the placeholders and draw records of the last draw_all (the loss has planned its
    kernels; holding them would keep the step's autograd graph alive).
    """
    _LAZY.clear()
    _DRAWN.clear()
    flush_draws(claimed=True)


def drawn_of(tensor) -> Optional[Drawn]:
    """The materialised draw a sample tensor (or a view sharing its storage start) is, or None."""
    if not _DRAWN or not isinstance(tensor, torch.Tensor):
        return None
    try:
        return _DRAWN.get(tensor.data_ptr())
    except RuntimeError:
        return None


def lazy_of(tensor) -> Optional[LazyDraw]:
    """
    The lazy draw a tensor (a placeholder, a broadcast view of one, or a batched view inside the
    particle vmap) stands for, or None.
    """
    if not _LAZY or not isinstance(tensor, torch.Tensor):
        return None
    functorch = torch._C._functorch
    base = tensor
    while functorch.is_batchedtensor(base):
        base = functorch.get_unwrapped(base)
    try:
        return _LAZY.get(base.data_ptr())
    except RuntimeError:  # tensors without storage
        return None


def _fusable_normal(distribution: Normal, N: int) -> bool:
    return (N >= 512 and N % 4 == 0 and distribution.loc.is_cuda and
            distribution.loc.dtype == torch.float32 and distribution.scale.dtype == torch.float32
            and switches.enabled("FUSE_DRAWS"))


def draw(distribution: Distribution, cfg: DrawConfig, lazy: bool = False) -> torch.Tensor:
    """
    K reparameterised draws of one guide factor: shape [K, *batch_shape, *event_shape].
    """
    cls = type(distribution)
    if (cfg.sharded or cfg.element_offset) and cls is not Normal:
        raise nat.NativeError(f"a data-sharded guide factor must be a Normal (got {cls.__name__}): "
                              "only the Normal sampler draws element slices of a global draw")
    if cfg.element_offset % 4:
        raise ValueError(f"element offset {cfg.element_offset} of a data-sharded factor is not a "
                         "multiple of 4 (mininf_amd.distributed.DataShard aligns slices)")
    if cls is Normal:
        shape = distribution.batch_shape
        N = max(1, int(shape.numel()))
        nat.require_device(distribution.loc, "guide Normal.loc")
        loc, loc_s = _flat_param(distribution.loc, N)
        scale, scale_s = _flat_param(distribution.scale, N)
        _inject(cfg, loc.device, N)
        if cfg.noise is None and lazy and _fusable_normal(distribution, N):
            # never read (recognised by its address; other uses re-trace with real draws)
            buffer = torch.empty(1, dtype=torch.float32, device=loc.device)
            placeholder = buffer.expand((cfg.K,) + tuple(shape))
            _LAZY[buffer.data_ptr()] = LazyDraw(cfg, loc, loc_s, scale, scale_s, N,
                                                torch.Size(shape), placeholder)
            return placeholder
        z = _NormalRsampleFn.apply(cfg, loc, loc_s, scale, scale_s)
        _DRAWN[z.data_ptr()] = Drawn(NORMAL_FAMILY, cfg, z, N)
        return z.reshape((cfg.K,) + tuple(shape))
    if cls is Beta:
        shape = distribution.batch_shape
        N = max(1, int(shape.numel()))
        conc = beta_concentration(distribution, N)
        nat.require_device(conc, "guide Beta concentration")
        _inject(cfg, conc.device, N)
        x = _BetaRsampleFn.apply(cfg, conc)
        _DRAWN[x.data_ptr()] = Drawn(BETA_FAMILY, cfg, x, N, _beta_dgrad(x, conc, cfg.K, N),
                                     conc)
        return x.reshape((cfg.K,) + tuple(shape))
    if cls is Gamma:
        shape = distribution.batch_shape
        N = max(1, int(shape.numel()))
        nat.require_device(distribution.concentration, "guide Gamma concentration")
        conc, conc_s, rate, rate_s = gamma_params(distribution, N)
        _inject(cfg, conc.device, N)   # standard draws g, [K, *shape]
        # a deferred exp transform of the guide's parameters runs before the sampler reads them
        # (no validation read has forced it when torch's argument validation is off, e.g. in a
        # captured step)
        fill_exp(conc)
        fill_exp(rate)
        x = _RsampleFn.apply(_GAMMA, cfg, conc, conc_s, rate, rate_s)
        return x.reshape((cfg.K,) + tuple(shape))
    for family in FAMILIES:
        if family.accepts(distribution):
            inputs, noise_shape, shape = family.prepare(distribution)
            _inject(cfg, inputs[family.sampler.params[0]].device, *noise_shape)
            _DRAWS[family.counter] += 1
            x = _RsampleFn.apply(family.sampler, cfg, *inputs)
            # (a [K, D] draw is returned as it is, without a view node)
            return x if x.shape[1:] == shape else x.reshape((cfg.K,) + shape)
    if cfg.noise is not None:
        return cfg.noise
    return distribution.rsample(torch.Size([cfg.K]))


def draw_all(approximation: Dict[str, Distribution], K: int, seed: int, step: int,
             particle_offset: int, noise: Optional[Dict[str, torch.Tensor]] = None,
             step_device: Optional[torch.Tensor] = None,
             lazy: bool = False,
             step_snapshot: Optional[torch.Tensor] = None,
             element_offsets: Optional[Dict[str, int]] = None) -> Dict[str, torch.Tensor]:
    """
    Draw every factor of a factorised guide (dict order = stream id order). With ``lazy``, large
    Normal factors become :class:`LazyDraw` placeholders evaluated inside the site kernels.
    ``element_offsets``: global index of element 0 of data-sharded factors (multiples of 4).
    """
    _LAZY.clear()
    _DRAWN.clear()
    _DRAWS.clear()
    flush_draws(claimed=True)
    samples = {}
    for stream_id, (name, factor) in enumerate(approximation.items()):
        cfg = DrawConfig(K=K, seed=seed, step=step, stream_id=stream_id,
                         particle_offset=particle_offset,
                         noise=None if noise is None else noise.get(name),
                         step_device=step_device, step_snapshot=step_snapshot,
                         element_offset=(element_offsets or {}).get(name, 0),
                         sharded=element_offsets is not None and name in element_offsets,
                         defer=lazy)
        samples[name] = draw(factor, cfg, lazy)
    return samples
