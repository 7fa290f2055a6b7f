"""
Deferred linear predictors: ``X @ theta`` inside a traced model without the [N, K] product.

The reference's regression models compute ``Normal(X @ theta, sigma)`` (``tests/test_mininf.py:13-18``,
``examples/minibatch.md:24-33``). Traced over K particles that matmul is a [N, K] GEMM whose output is
only ever read by the site's log density. While :func:`mininf_amd.particles.trace_particles` runs the
model, :class:`DeferredMatmul` (a ``TorchFunctionMode``) intercepts ``matmul(X, theta)`` for an
observed 2-D ``X`` and a per-particle 1-D ``theta`` and returns a *placeholder*: a batched tensor of
the right shape backed by a zero-stride zero, costing no memory and no kernel. The particle tracer
turns a Normal / Bernoulli-logits site whose location / logits is such a placeholder into a fused
linear site (``mi_linear_forward``: the product is evaluated inside the site kernel). So are the
count regressions: a Binomial / NegativeBinomial whose ``logits`` is a placeholder, and a Poisson
whose ``rate`` is ``exp`` of one -- ``torch.exp`` / ``Tensor.exp`` of a placeholder is a placeholder
tagged with the *link* ``exp`` (the log link of the regression), which materialises to ``exp`` of
the real product.

The multi-class regression ``Categorical(logits=X @ Theta)`` with a per-particle matrix ``Theta``
[P, C] is deferred the same way (``torch.matmul`` only; the placeholder has shape [N, C]).
``Categorical.__init__`` normalises its logits, ``logits - logits.logsumexp(dim=-1, keepdim=True)``:
``logsumexp`` of such a placeholder over its last dimension (``keepdim=True``) is a placeholder
[N, 1] with the link ``logsumexp``, the difference of the two (and ``log_softmax`` over the last
dimension) one with the link ``log_softmax``; a ``log_softmax`` placeholder normalises again the
same way (``Categorical(logits=torch.log_softmax(eta, -1))``). The tracer turns a Categorical site whose logits are
an identity or ``log_softmax`` placeholder into a fused softmax site
(``mi_softmax_linear_forward``).

Semantics are preserved for every other use: any torch operation that reads a placeholder's values
(anything but shape queries and broadcasting views) first *materialises* it -- the real
``torch.matmul(X, theta)`` is computed at that point, exactly as the model wrote it -- and the
operation runs on the real tensor. A placeholder therefore never leaks a wrong value into the model.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch
from torch.overrides import TorchFunctionMode
from torch.utils._pytree import tree_map

from . import guide as _guide
from .guide import lazy_of

_functorch = torch._C._functorch

_MATMULS = {torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__, torch.mv, torch.Tensor.mv}
_MVS = {torch.mv, torch.Tensor.mv}

# Operations that only read metadata (never values) pass a placeholder through unchanged.
_METADATA = {
    torch.Tensor.size, torch.Tensor.dim, torch.Tensor.ndimension, torch.Tensor.numel,
    torch.Tensor.__len__, torch.Tensor.is_floating_point, torch.Tensor.is_complex,
    torch.Tensor.stride, torch.Tensor.element_size,
    torch.Tensor.shape.__get__, torch.Tensor.dtype.__get__, torch.Tensor.device.__get__,
    torch.Tensor.ndim.__get__, torch.Tensor.requires_grad.__get__, torch.Tensor.is_cuda.__get__,
    torch.Tensor.layout.__get__, torch.Tensor.is_sparse.__get__, torch.Tensor.grad_fn.__get__,
    torch.Tensor.is_leaf.__get__, torch.Tensor.names.__get__,
}

# exp of an identity-link placeholder is a placeholder with the link "exp" (Poisson's log link).
_EXPS = {torch.exp, torch.Tensor.exp}

# The normalisation of Categorical's logits over a [N, C] placeholder (see the module docstring).
_LOGSUMEXPS = {torch.logsumexp, torch.Tensor.logsumexp}
_SUBS = {torch.sub, torch.Tensor.sub, torch.Tensor.__sub__}
_LOG_SOFTMAXES = {torch.log_softmax, torch.Tensor.log_softmax, torch.nn.functional.log_softmax}

# Most categories of a deferred `X @ Theta` (MI_SOFTMAX_LINEAR_MAX_C of include/mininf_amd.h).
MAX_CATEGORIES = 32

# Broadcasting views of a placeholder are placeholders of the broadcast shape (and the same link).
_BROADCASTS = {torch.broadcast_tensors, torch.Tensor.expand, torch.Tensor.expand_as,
               torch.Tensor.broadcast_to, torch.broadcast_to}


class NeedsDraws(Exception):
    """
    Raised while tracing when the model uses a lazy guide draw (:class:`mininf_amd.guide.LazyDraw`)
    in an operation other than a site parameter / value: the loss then re-traces with real draws.
    """



def _leaves(args, kwargs):
    """The tensors of a torch function call's arguments (lists, tuples and dicts walked; the
    pytree machinery costs tens of microseconds per call on this path)."""
    stack = [args, kwargs]
    while stack:
        x = stack.pop()
        if isinstance(x, torch.Tensor):
            yield x
        elif isinstance(x, (list, tuple)):
            stack.extend(x)
        elif isinstance(x, dict):
            stack.extend(x.values())

@dataclasses.dataclass
class Deferred:
    """
    ``root``: the deferred ``X @ theta`` (``X`` [N, P] observed, ``theta`` batched [P]); a derived
    placeholder is ``root`` broadcast to ``shape``, then passed through ``link`` ("identity" or
    "exp"). With ``theta`` batched [P, C] the root has shape [N, C], and the links "logsumexp"
    (over the last dimension, kept) and "log_softmax" are applied before the broadcast.
    """
    X: torch.Tensor
    theta: torch.Tensor
    shape: torch.Size
    root: Optional["Deferred"] = None
    real: Optional[torch.Tensor] = None
    link: str = "identity"
    # the normalisations behind a "log_softmax" placeholder (or under a "logsumexp" one), in order:
    # "sub" (x - x.logsumexp(-1, keepdim=True), as Categorical.__init__ writes it) or "log_softmax";
    # Categorical(logits=torch.log_softmax(eta, -1)) normalises twice
    steps: Tuple[str, ...] = ()


class DeferredMatmul(TorchFunctionMode):
    """
    Active while a model is traced over particles (inside ``vmap``); see the module docstring.
    """
    require_device = True   # defer only device matmuls (the fused kernel's operands)

    def __init__(self, K: int, defer_matmul: bool = True) -> None:
        super().__init__()
        self.K = K
        self.defer_matmul = defer_matmul
        self.deferred: Dict[int, Deferred] = {}
        self._keep: List[torch.Tensor] = []   # placeholders stay alive: ids are never reused
        self._bypass = False

    # ---- helpers ---------------------------------------------------------------------------
    def lookup(self, tensor: Any) -> Optional[Deferred]:
        if isinstance(tensor, torch.Tensor):
            return self.deferred.get(id(tensor))
        return None

    def _eligible(self, args, kwargs, matrix: bool = False) -> bool:
        """``matrix``: the call is a matmul (not ``mv``), which also takes a [P, C] theta."""
        if kwargs or len(args) != 2:
            return False
        X, theta = args
        if not (isinstance(X, torch.Tensor) and isinstance(theta, torch.Tensor)):
            return False
        if self.lookup(X) is not None or self.lookup(theta) is not None:
            return False
        if not self.defer_matmul or lazy_of(X) is not None or lazy_of(theta) is not None:
            return False
        return (not _functorch.is_batchedtensor(X) and X.dim() == 2 and
                (X.is_cuda or not self.require_device) and
                X.dtype == torch.float32 and not X.requires_grad and
                _functorch.is_batchedtensor(theta) and
                (theta.dim() == 1 or (matrix and theta.dim() == 2 and
                                      2 <= theta.shape[1] <= MAX_CATEGORIES)) and
                theta.dtype == torch.float32 and theta.shape[0] == X.shape[1] and
                X.shape[1] <= 64 and X.shape[0] > 0)

    def _placeholder(self, like: torch.Tensor, shape: torch.Size, info: Deferred) -> torch.Tensor:
        level = _functorch.maybe_get_level(like)
        # never read (any value-reading use materialises the product): no initialising kernel
        base = torch.empty((), dtype=torch.float32, device=info.X.device)
        base = base.expand((self.K,) + tuple(shape))
        out = _functorch._add_batch_dim(base, 0, level)
        self.deferred[id(out)] = info
        self._keep.append(out)
        return out

    def materialize(self, tensor: torch.Tensor) -> torch.Tensor:
        """
        The real value of a placeholder (computed once), or ``tensor`` itself.
        """
        info = self.lookup(tensor)
        if info is None:
            return tensor
        root = info.root or info
        if root.real is None:
            _guide.flush_draws()   # theta may be a guide draw not launched yet
            self._bypass = True
            try:
                root.real = torch.matmul(root.X, root.theta)
            finally:
                self._bypass = False
        if info.root is None:
            return root.real
        if info.real is None:
            self._bypass = True
            try:
                if info.link in ("logsumexp", "log_softmax"):
                    real = root.real
                    for step in info.steps:   # each as the model wrote it
                        real = torch.log_softmax(real, -1) if step == "log_softmax" else \
                            real - real.logsumexp(dim=-1, keepdim=True)
                    if info.link == "logsumexp":
                        real = real.logsumexp(dim=-1, keepdim=True)
                    info.real = real.expand(info.shape)
                else:
                    info.real = root.real.expand(info.shape)
                    if info.link == "exp":
                        info.real = info.real.exp()
            finally:
                self._bypass = False
        return info.real

    # ---- the mode ----------------------------------------------------------------------------
    def __torch_function__(self, func: Callable, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if self._bypass:
            return func(*args, **kwargs)
        if func in _MATMULS and self._eligible(args, kwargs, func not in _MVS):
            X, theta = args
            info = Deferred(X=X, theta=theta, shape=torch.Size((X.shape[0],) + tuple(theta.shape[1:])))
            return self._placeholder(theta, info.shape, info)
        if not self.deferred and not _guide._LAZY and \
                (not _guide._PENDING_DRAWS or func in _METADATA or func in _BROADCASTS):
            # no placeholder exists, and no pending draw is read by this call: nothing to do
            return func(*args, **kwargs)
        touched = []
        lazy = []
        for x in _leaves(args, kwargs):
            info = self.lookup(x)
            if info is not None:
                touched.append(info)
            elif lazy_of(x) is not None:
                lazy.append(x)
            elif func not in _METADATA and func not in _BROADCASTS and \
                    _guide.pending_draw(x) is not None:
                # the model reads a guide draw whose launch was left to the loss's planning
                _guide.flush_draws()
        if not touched and not lazy:
            return func(*args, **kwargs)
        if func in _METADATA:
            return func(*args, **kwargs)
        if func is torch.Tensor.type_as and len(args) == 2 and self.lookup(args[0]) is None and \
                lazy_of(args[0]) is None:
            # `x.type_as(placeholder)` reads the placeholder's dtype and device only (Binomial and
            # NegativeBinomial cast their total_count to their logits' type this way)
            return func(*args, **kwargs)
        if lazy and func not in _BROADCASTS:
            raise NeedsDraws(getattr(func, "__name__", str(func)))
        if not touched:
            return func(*args, **kwargs)
        if func in _BROADCASTS:
            out = func(*args, **kwargs)
            inputs = args[0] if func is torch.broadcast_tensors and len(args) == 1 and \
                isinstance(args[0], (list, tuple)) else args
            if func is torch.broadcast_tensors:
                outs = list(out)
                for src, dst in zip(inputs, outs):
                    self._derive(src, dst)
            else:
                self._derive(args[0], out)
            return out
        if func in _EXPS and len(args) == 1 and not kwargs and touched[0].link == "identity":
            info = touched[0]
            root = info.root or info
            derived = Deferred(X=root.X, theta=root.theta, shape=torch.Size(args[0].shape),
                               root=root, link="exp")
            return self._placeholder(args[0], derived.shape, derived)
        derived = self._softmax_link(func, args, kwargs)
        if derived is not None:
            return self._placeholder(args[0], derived.shape, derived)
        args, kwargs = tree_map(lambda x: self.materialize(x) if self.lookup(x) else x,
                                (args, kwargs))
        return func(*args, **kwargs)

    def _softmax_link(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """
        The derived placeholder of ``logsumexp(ph, -1, keepdim=True)``, ``ph - lse`` or
        ``log_softmax(ph, -1)`` over a [.., N, C] identity placeholder ``ph``; None for anything else.
        """
        info = self.lookup(args[0]) if args else None
        if info is None or info.link not in ("identity", "log_softmax") or \
                (info.root or info).theta.dim() != 2:
            return None
        root = info.root or info
        shape = tuple(args[0].shape)

        def last_dim(extra) -> bool:
            rest = dict(kwargs)
            rest.pop("_stacklevel", None)
            dim = args[1] if len(args) > 1 else rest.pop("dim", None)
            if len(args) > 2 or isinstance(dim, bool) or not isinstance(dim, int):
                return False
            return dim in (-1, len(shape) - 1) and rest == extra

        if func in _LOGSUMEXPS and last_dim({"keepdim": True}):
            return Deferred(X=root.X, theta=root.theta, shape=torch.Size(shape[:-1] + (1,)),
                            root=root, link="logsumexp", steps=info.steps)
        if func in _LOG_SOFTMAXES and (last_dim({}) or last_dim({"dtype": None})):
            return Deferred(X=root.X, theta=root.theta, shape=torch.Size(shape), root=root,
                            link="log_softmax", steps=info.steps + ("log_softmax",))
        if func in _SUBS and len(args) == 2 and not kwargs:
            other = self.lookup(args[1])
            if other is not None and other.link == "logsumexp" and other.root is root and \
                    other.steps == info.steps and tuple(args[1].shape) == shape[:-1] + (1,):
                return Deferred(X=root.X, theta=root.theta, shape=torch.Size(shape), root=root,
                                link="log_softmax", steps=info.steps + ("sub",))
        return None

    def _derive(self, src: Any, dst: torch.Tensor) -> None:
        info = self.lookup(src)
        if info is None or not isinstance(dst, torch.Tensor):
            return
        root = info.root or info
        self.deferred[id(dst)] = Deferred(X=root.X, theta=root.theta,
                                          shape=torch.Size(dst.shape), root=root, link=info.link,
                                          steps=info.steps)
        self._keep.append(dst)
