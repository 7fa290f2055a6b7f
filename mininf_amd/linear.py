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

A parameter indexed by a group label, ``alpha[group]`` with a per-particle table ``alpha`` [G] and
an observed 1-D integer ``group`` [N] (``Tensor.__getitem__`` or ``index_select`` over dimension
0), is deferred the same way (:class:`DeferredGather`): the placeholder [N] stays one through
broadcasting views, through ``add`` / ``sub`` / ``mul`` (and their reflected forms) with a Python
number or a per-particle scalar -- they compose the affine predictor ``shift + mult * alpha[group]``
-- and through ``exp`` of it. The tracer turns a Normal / Bernoulli-logits / Poisson site whose
parameter is such a placeholder into a gathered site (``mi_gather_site_forward``: the [K, N] gather
and its scatter-add backward never run). ``MININF_AMD_DEFER_GATHER=0`` turns this off.

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
from . import switches
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


# A gather `table[index]` over dimension 0, and the arithmetic that keeps its placeholder one.
_GETITEMS = {torch.Tensor.__getitem__}
_INDEX_SELECTS = {torch.index_select, torch.Tensor.index_select}
_ADDS = {torch.add: False, torch.Tensor.add: False, torch.Tensor.__add__: False,
         torch.Tensor.__radd__: True}
_MULS = {torch.mul: False, torch.Tensor.mul: False, torch.Tensor.__mul__: False,
         torch.Tensor.__rmul__: True}
_SUBTRACTS = {torch.sub: False, torch.Tensor.sub: False, torch.Tensor.__sub__: False,
              torch.Tensor.__rsub__: True}   # True: reflected, func(x, y) = y op x


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


@dataclasses.dataclass
class DeferredGather:
    """
    A placeholder of ``link(shift + mult * table[index])`` broadcast to ``shape``: ``table`` batched
    [G], ``index`` an observed 1-D integer tensor [N], ``shift`` / ``mult`` None (0 / 1), a Python
    number or a per-particle (batched 0-d) tensor, ``link`` "identity" or "exp". ``parent`` and
    ``replay`` materialise it: the parent's real value passed through the operation as the model
    wrote it (the root: the gather itself). ``chain`` lists those operations, in order, for a
    planner that has to put the gather back after the trace: ("add" | "sub" | "mul", c, left) with
    the placeholder the left operand or not.
    """
    table: torch.Tensor
    index: torch.Tensor
    shape: torch.Size
    shift: Any = None
    mult: Any = None
    link: str = "identity"
    parent: Optional["DeferredGather"] = None
    replay: Optional[Callable] = None
    real: Optional[torch.Tensor] = None
    chain: Tuple[Tuple[str, Any, bool], ...] = ()


class DeferredMatmul(TorchFunctionMode):
    """
    Active while a model is traced over particles (inside ``vmap``); see the module docstring.
    """
    require_device = True   # defer only device matmuls (the fused kernel's operands)

    def __init__(self, K: int, defer_matmul: bool = True,
                 defer_gather: Optional[bool] = None) -> None:
        super().__init__()
        self.K = K
        self.defer_matmul = defer_matmul
        self.defer_gather = switches.enabled("DEFER_GATHER") if defer_gather is None \
            else defer_gather
        self.deferred: Dict[int, Deferred] = {}
        self.gathers: Dict[int, DeferredGather] = {}
        # per-particle scalars broadcast beside a gather placeholder (Normal's broadcast_all of
        # loc and scale): the broadcast view -> the scalar it came from
        self.sources: Dict[int, torch.Tensor] = {}
        self._keep: List[torch.Tensor] = []   # placeholders stay alive: ids are never reused
        self._bypass = False

    # ---- helpers ---------------------------------------------------------------------------
    def lookup(self, tensor: Any) -> Optional[Deferred]:
        if isinstance(tensor, torch.Tensor):
            return self.deferred.get(id(tensor))
        return None

    def lookup_gather(self, tensor: Any) -> Optional[DeferredGather]:
        if isinstance(tensor, torch.Tensor):
            return self.gathers.get(id(tensor))
        return None

    def _gather_call(self, func: Callable, args, kwargs):
        """(table, index) of a call that is ``table[index]`` over a per-particle 1-D float32
        table and an observed 1-D integer index, or None."""
        if func in _GETITEMS:
            if kwargs or len(args) != 2:
                return None
            table, index = args
        elif func in _INDEX_SELECTS:
            names = ("input", "dim", "index")
            if len(args) > 3 or any(key not in names[len(args):] for key in kwargs):
                return None
            full = list(args) + [kwargs.get(name) for name in names[len(args):]]
            table, dim, index = full
            if isinstance(dim, bool) or not isinstance(dim, int) or dim not in (0, -1):
                return None
        else:
            return None
        if not (isinstance(table, torch.Tensor) and isinstance(index, torch.Tensor)):
            return None
        if self.lookup(table) is not None or self.lookup_gather(table) is not None or \
                lazy_of(table) is not None or lazy_of(index) is not None:
            return None
        if not (_functorch.is_batchedtensor(table) and table.dim() == 1 and
                table.dtype == torch.float32 and table.shape[0] > 0 and
                (table.is_cuda or not self.require_device)):
            return None
        if _functorch.is_batchedtensor(index) or index.dim() != 1 or index.shape[0] == 0 or \
                index.dtype not in (torch.int64, torch.int32) or index.requires_grad or \
                index.device != table.device:
            return None
        return table, index

    def _gather_placeholder(self, like: torch.Tensor, info: DeferredGather) -> torch.Tensor:
        level = _functorch.maybe_get_level(like)
        base = torch.empty((), dtype=torch.float32, device=info.table.device)
        base = base.expand((self.K,) + tuple(info.shape))
        out = _functorch._add_batch_dim(base, 0, level)
        self.gathers[id(out)] = info
        self._keep.append(out)
        return out

    def _scalar(self, x: Any) -> bool:
        """A Python number or a per-particle float32 scalar: a term of the affine predictor."""
        if isinstance(x, bool):
            return False
        if isinstance(x, (int, float)):
            return True
        return isinstance(x, torch.Tensor) and _functorch.is_batchedtensor(x) and x.dim() == 0 and \
            x.dtype == torch.float32 and self.lookup(x) is None and \
            self.lookup_gather(x) is None and lazy_of(x) is None

    def _affine(self, func: Callable, args, kwargs) -> Optional[torch.Tensor]:
        """The placeholder of ``ph + c``, ``ph - c``, ``c - ph`` or ``ph * c`` for an identity-link
        gather placeholder ``ph`` and a scalar ``c``; None for anything else."""
        kind = "add" if func in _ADDS else "mul" if func in _MULS else \
            "sub" if func in _SUBTRACTS else None
        if kind is None or kwargs or len(args) != 2:
            return None
        reflected = (_ADDS if kind == "add" else _MULS if kind == "mul" else _SUBTRACTS)[func]
        x, y = (args[1], args[0]) if reflected else args   # the call computes x op y
        if self.lookup_gather(x) is not None and self._scalar(y):
            ph, c, left = x, y, True
        elif self.lookup_gather(y) is not None and self._scalar(x):
            ph, c, left = y, x, False
        else:
            return None
        info = self.lookup_gather(ph)
        if info.link != "identity":
            return None
        shift, mult = info.shift, info.mult
        self._bypass = True   # (per-particle scalars: [K] operations)
        try:
            if kind == "add":
                shift = c if shift is None else shift + c
            elif kind == "sub" and left:
                shift = -c if shift is None else shift - c
            elif kind == "sub":
                shift = c if shift is None else c - shift
                mult = -1.0 if mult is None else -mult
            else:
                shift = None if shift is None else shift * c
                mult = c if mult is None else mult * c
        finally:
            self._bypass = False

        def replay(real, c=c, left=left, func=func, reflected=reflected):
            operands = (real, c) if left else (c, real)
            return func(*(operands[::-1] if reflected else operands))
        derived = DeferredGather(table=info.table, index=info.index, shape=info.shape, shift=shift,
                                 mult=mult, link="identity", parent=info, replay=replay,
                                 chain=info.chain + ((kind, c, left),))
        return self._gather_placeholder(ph, derived)

    def _materialize_gather(self, info: DeferredGather) -> torch.Tensor:
        if info.real is None:
            if info.parent is None:
                _guide.flush_draws()   # the table may be a guide draw not launched yet
            else:
                real = self._materialize_gather(info.parent)
            self._bypass = True
            try:
                info.real = info.replay() if info.parent is None else info.replay(real)
            finally:
                self._bypass = False
        return info.real

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
        gathered = self.lookup_gather(tensor)
        if gathered is not None:
            return self._materialize_gather(gathered)
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
        if self.defer_gather and (func in _GETITEMS or func in _INDEX_SELECTS):
            call = self._gather_call(func, args, kwargs)
            if call is not None:
                table, index = call
                info = DeferredGather(table=table, index=index, shape=torch.Size(index.shape),
                                      replay=lambda: func(*args, **kwargs))
                return self._gather_placeholder(table, info)
        if not self.deferred and not self.gathers and not _guide._LAZY and \
                (not _guide._PENDING_DRAWS or func in _METADATA or func in _BROADCASTS):
            # no placeholder exists, and no pending draw is read by this call: nothing to do
            return func(*args, **kwargs)
        touched = []
        lazy = []
        gathered = []
        for x in _leaves(args, kwargs):
            info = self.lookup(x)
            if info is not None:
                touched.append(info)
            elif self.lookup_gather(x) is not None:
                gathered.append(self.lookup_gather(x))
            elif lazy_of(x) is not None:
                lazy.append(x)
            elif func not in _METADATA and func not in _BROADCASTS and \
                    _guide.pending_draw(x) is not None:
                # the model reads a guide draw whose launch was left to the loss's planning
                _guide.flush_draws()
        if not touched and not lazy and not gathered:
            return func(*args, **kwargs)
        if func in _METADATA:
            return func(*args, **kwargs)
        if func is torch.Tensor.type_as and len(args) == 2 and self.lookup(args[0]) is None and \
                self.lookup_gather(args[0]) is None and lazy_of(args[0]) is None:
            # `x.type_as(placeholder)` reads the placeholder's dtype and device only (Binomial and
            # NegativeBinomial cast their total_count to their logits' type this way)
            return func(*args, **kwargs)
        if lazy and func not in _BROADCASTS:
            raise NeedsDraws(getattr(func, "__name__", str(func)))
        if not touched and not gathered:
            return func(*args, **kwargs)
        if func in _BROADCASTS:
            out = func(*args, **kwargs)
            inputs = args[0] if func is torch.broadcast_tensors and len(args) == 1 and \
                isinstance(args[0], (list, tuple)) else args
            if func is torch.broadcast_tensors:
                outs = list(out)
                for src, dst in zip(inputs, outs):
                    self._derive(src, dst)
                    if gathered and isinstance(src, torch.Tensor) and src.dim() == 0 and \
                            self.lookup(src) is None and self.lookup_gather(src) is None:
                        self.sources[id(dst)] = src
                        self._keep.append(dst)
            else:
                self._derive(args[0], out)
            return out
        if gathered and not touched:
            if func in _EXPS and len(args) == 1 and not kwargs and gathered[0].link == "identity":
                info = gathered[0]
                derived = DeferredGather(table=info.table, index=info.index, shape=info.shape,
                                         shift=info.shift, mult=info.mult, link="exp", parent=info,
                                         replay=lambda real: func(real), chain=info.chain)
                return self._gather_placeholder(args[0], derived)
            out = self._affine(func, args, kwargs)
            if out is not None:
                return out
        if not touched:
            args, kwargs = tree_map(lambda x: self.materialize(x), (args, kwargs))
            return func(*args, **kwargs)
        if func in _EXPS and len(args) == 1 and not kwargs and touched[0].link == "identity":
            info = touched[0]
            root = info.root or info
            derived = Deferred(X=root.X, theta=root.theta, shape=torch.Size(args[0].shape),
                               root=root, link="exp")
            return self._placeholder(args[0], derived.shape, derived)
        derived = self._softmax_link(func, args, kwargs)
        if derived is not None:
            return self._placeholder(args[0], derived.shape, derived)
        args, kwargs = tree_map(lambda x: self.materialize(x), (args, kwargs))
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
        gathered = self.lookup_gather(src)
        if gathered is not None and isinstance(dst, torch.Tensor):
            shape = torch.Size(dst.shape)
            self.gathers[id(dst)] = DeferredGather(
                table=gathered.table, index=gathered.index, shape=shape, shift=gathered.shift,
                mult=gathered.mult, link=gathered.link, parent=gathered,
                replay=lambda real: real.expand(shape), chain=gathered.chain)
            self._keep.append(dst)
            return
        info = self.lookup(src)
        if info is None or not isinstance(dst, torch.Tensor):
            return
        root = info.root or info
        self.deferred[id(dst)] = Deferred(X=root.X, theta=root.theta,
                                          shape=torch.Size(dst.shape), root=root, link=info.link,
                                          steps=info.steps)
        self._keep.append(dst)
