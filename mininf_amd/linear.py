"""
Deferred predictors: ``X @ theta`` and ``alpha[group]`` inside a traced model without the [N, K]
product or gather.

The reference's regression models compute ``Normal(X @ theta, sigma)`` (``tests/test_mininf.py:13-18``,
``examples/minibatch.md:24-33``). Traced over K particles that matmul is a [N, K] GEMM whose output is
only ever read by the site's log density. While :func:`mininf_amd.particles.trace_particles` runs the
model, :class:`DeferredMatmul` (a ``TorchFunctionMode``) answers such a call with a *placeholder*: a
batched tensor of the right shape backed by a zero-stride scalar that is never read, costing no
memory and no kernel, with one record (:class:`Deferred`) in the mode's table. The tracer turns a
site whose parameter is still a placeholder into a fused site, whose kernel evaluates the predictor
(``mi_linear_forward``, ``mi_softmax_linear_forward``, ``mi_gather_site_forward``).

**Roots.** ``"matmul"``: ``matmul`` / ``mv`` of an observed float32 ``X`` [N, P] and a per-particle
``theta`` [P] or (``matmul`` only) ``Theta`` [P, C], C <= ``MAX_CATEGORIES``: a placeholder [N] or
[N, C]. ``"gather"``: ``table[index]`` (``__getitem__``, or ``index_select`` over dimension 0) of a
per-particle float32 ``table`` [G] and an observed 1-D integer ``index`` [N]. The switches
``MININF_AMD_DEFER_MATMUL=0`` / ``MININF_AMD_DEFER_GATHER=0`` turn them off.

**Derivations.** A call on a placeholder that a site kernel can still evaluate returns another
placeholder, whose record holds its parent and the replay of the call on the parent's real value:

====================================  ======  =====================  ===========
call                                  kind    link of ``ph``         new link
====================================  ======  =====================  ===========
broadcasting views                    either  any                    unchanged
``exp(ph)``                           either  identity               exp
``ph + c``, ``ph - c``, ``ph * c``    gather  identity               identity
``gather + matmul`` (``defer_sum``)   both    identity, identity     identity
``gather * z`` (``defer_slope``)      gather  identity (root)        (a product)
``gather + product``                  gather  identity               identity
``ph.logsumexp(-1, keepdim=True)``    matmul  identity, log_softmax  logsumexp
``log_softmax(ph, -1)``               matmul  identity, log_softmax  log_softmax
``ph - lse``                          matmul  identity, log_softmax  log_softmax
====================================  ======  =====================  ===========

``exp`` is the log link of a Poisson rate. ``c`` is a Python number or a per-particle scalar, in the
plain and the reflected forms: they compose ``shift + mult * table[index]``. The last three apply to
a [.., N, C] placeholder of ``X @ Theta`` and are how ``Categorical.__init__`` normalises its logits
(``logits - logits.logsumexp(dim=-1, keepdim=True)``: ``lse`` is the logsumexp placeholder of the
same root after the same normalisations) and how a model does (``torch.log_softmax(eta, -1)``).
With ``defer_sum`` the sum (``add`` in all its forms, either order) of a gather placeholder with any
affine chain and the root placeholder of ``X @ theta`` for a vector ``theta`` of at most
``MAX_SUM_FEATURES`` entries over the same N is a gather-kind record that also carries ``X``,
``theta`` and which operand stood on the left (``mi_gather_linear_forward``). It still takes
``+ c``, ``- c`` (composed into ``shift``, remembered in ``post``) and ``exp``; ``* c`` and ``c - ...``
(which would negate the linear term) materialise, like a second gather or product.
With ``defer_slope`` the product (``mul`` in all its forms, either order) of a root gather
placeholder ``beta[index]`` and an observed float32 column ``z`` [N] is a *product* placeholder
(kind ``"slope"``) whose only accepted use is as a summand: the sum (``add``, either order) of an
identity-link gather record -- any affine chain, with or without the ``X @ theta`` above, holding
fewer than ``MAX_SLOPES`` slopes -- and a product whose gather used the same index tensor object is
a gather-kind record with one more slope (``mi_gather_slopes_forward``). A record that holds slopes
still takes ``X @ theta`` once, ``+ c``, ``- c`` and ``exp``; ``summands`` remembers every operation
after the gather's own chain in the model's order and sides. Any other call on a product first
makes ``table[index] * z`` real, in the order the model wrote it.
Metadata queries and ``x.type_as(ph)`` read no values and pass a placeholder through.

**Anything else materialises.** Every other torch operation that meets a placeholder first gets its
real value -- the root's call as the model wrote it, computed once, then the replay of each
derivation -- and runs on the real tensor, so a placeholder never leaks a wrong value into the
model. After the trace, :func:`put_back` does the same for a site a planner's kernel cannot take.
"""
from __future__ import annotations

import contextlib
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

# Broadcasting views of a placeholder are placeholders of the broadcast shape (and the same link).
_BROADCASTS = {torch.broadcast_tensors, torch.Tensor.expand, torch.Tensor.expand_as,
               torch.Tensor.broadcast_to, torch.broadcast_to}

_GETITEMS = {torch.Tensor.__getitem__}
_INDEX_SELECTS = {torch.index_select, torch.Tensor.index_select}

# The functions of the derivations. Arithmetic: True for a reflected form, func(x, y) = y op x.
_EXPS = {torch.exp, torch.Tensor.exp}
_LOGSUMEXPS = {torch.logsumexp, torch.Tensor.logsumexp}
_LOG_SOFTMAXES = {torch.log_softmax, torch.Tensor.log_softmax, torch.nn.functional.log_softmax}
_ADDS = {torch.add: False, torch.Tensor.add: False, torch.Tensor.__add__: False,
         torch.Tensor.__radd__: True}
_MULS = {torch.mul: False, torch.Tensor.mul: False, torch.Tensor.__mul__: False,
         torch.Tensor.__rmul__: True}
_SUBS = {torch.sub: False, torch.Tensor.sub: False, torch.Tensor.__sub__: False,
         torch.Tensor.__rsub__: True}
_ARITHMETIC = {"add": _ADDS, "sub": _SUBS, "mul": _MULS}

# Most categories of a deferred `X @ Theta` (MI_SOFTMAX_LINEAR_MAX_C of include/mininf_amd.h).
MAX_CATEGORIES = 32
# Most columns of X in a deferred ``alpha[group] + X @ theta`` (MI_GATHER_LINEAR_MAX_P).
MAX_SUM_FEATURES = 32
# Most slope terms ``beta[group] * z`` of one deferred predictor (MI_GATHER_MAX_SLOPES).
MAX_SLOPES = 4


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


def _last_dim(args, kwargs, ndim: int, extra: dict) -> bool:
    """Whether a reduction ``func(ph, dim, **extra)`` runs over the last of ``ndim`` dimensions."""
    rest = dict(kwargs)
    rest.pop("_stacklevel", None)
    dim = args[1] if len(args) > 1 else rest.pop("dim", None)
    if len(args) > 2 or isinstance(dim, bool) or not isinstance(dim, int):
        return False
    return dim in (-1, ndim - 1) and rest == extra


@dataclasses.dataclass
class Deferred:
    """
    The record of one placeholder of ``shape`` (without the particle axis): ``replay`` applied to
    the real value of ``parent`` gives its own, cached in ``real``; a root has no parent and its
    ``replay()`` is the call the model wrote. ``link`` is what it stands for, as a function of the
    root's predictor (see the module docstring).

    ``"matmul"``: ``X`` and ``theta`` as the model passed them. ``steps`` lists the normalisations
    behind a "log_softmax" placeholder (or under a "logsumexp" one), in order: "sub"
    (``x - x.logsumexp(-1, keepdim=True)``) or "log_softmax". Every derived record hangs off its
    root: its replay is the whole path from the product.

    ``"gather"``: ``link(shift + mult * table[index] [+ X @ theta])`` with ``shift`` / ``mult`` None (0 / 1), a
    Python number or a per-particle (batched 0-d) tensor. ``chain`` lists the affine operations, in
    order, for :func:`put_back`: ("add" | "sub" | "mul", c, left), the placeholder the left
    operand or not. After a deferred sum ``X`` and ``theta`` are the product's, ``linear_left``
    says whether the gather was the sum's left operand and ``post`` lists the later scalar
    operations like ``chain``. ``slopes`` lists the slope terms of the predictor, (table, z, whether
    the table was the product's left operand), and ``summands`` every operation after ``chain`` in
    the model's order: ("slope", position in ``slopes``, left), ("linear", None, left) or a scalar
    operation like those of ``chain``, ``left`` saying whether the record was the left operand.

    ``"slope"``: the product ``table[index] * z`` of a root gather placeholder (``parent``) and an
    observed column ``z``; ``slope_left`` says whether the gather was the product's left operand.
    """
    kind: str
    shape: torch.Size
    link: str = "identity"
    parent: Optional["Deferred"] = None
    replay: Optional[Callable] = None
    real: Optional[torch.Tensor] = None
    X: Optional[torch.Tensor] = None
    theta: Optional[torch.Tensor] = None
    steps: Tuple[str, ...] = ()
    table: Optional[torch.Tensor] = None
    index: Optional[torch.Tensor] = None
    shift: Any = None
    mult: Any = None
    chain: Tuple[Tuple[str, Any, bool], ...] = ()
    linear_left: bool = True
    post: Tuple[Tuple[str, Any, bool], ...] = ()
    slopes: Tuple[Tuple[torch.Tensor, torch.Tensor, bool], ...] = ()
    summands: Tuple[Tuple[str, Any, bool], ...] = ()
    z: Optional[torch.Tensor] = None
    slope_left: bool = True

    @property
    def root(self) -> "Deferred":
        info = self
        while info.parent is not None:
            info = info.parent
        return info

    def derived(self, **changes) -> "Deferred":
        """A record derived from this one: a copy with ``changes`` and no real value yet."""
        new = object.__new__(Deferred)   # (dataclasses.replace costs microseconds on every trace)
        new.__dict__.update(self.__dict__)
        new.__dict__.update(changes, parent=self, real=None)
        return new


def _matmul_derived(root: Deferred, shape, link: str, steps: Tuple[str, ...] = ()) -> Deferred:
    """The record of ``link`` of the product ``root`` after ``steps``, broadcast to ``shape``."""
    shape = torch.Size(shape)

    def replay(real):
        for step in steps:   # each as the model wrote it
            real = torch.log_softmax(real, -1) if step == "log_softmax" else \
                real - real.logsumexp(dim=-1, keepdim=True)
        if link == "logsumexp":
            real = real.logsumexp(dim=-1, keepdim=True)
        real = real.expand(shape)
        return real.exp() if link == "exp" else real
    return root.derived(shape=shape, link=link, steps=steps, replay=replay)


class DeferredMatmul(TorchFunctionMode):
    """
    Active while a model is traced over particles (inside ``vmap``); see the module docstring.
    """
    require_device = True   # defer only device operands (the fused kernels')

    def __init__(self, K: int, defer_matmul: bool = True,
                 defer_gather: Optional[bool] = None, defer_sum: bool = False,
                 defer_slope: bool = False) -> None:
        super().__init__()
        self.K = K
        self.defer_matmul = defer_matmul
        self.defer_gather = switches.enabled("DEFER_GATHER") if defer_gather is None \
            else defer_gather
        # (the sum of both predictors needs both deferred)
        self.defer_sum = bool(defer_sum and self.defer_matmul and self.defer_gather)
        # (a slope is a summand beside a deferred gather)
        self.defer_slope = bool(defer_slope and self.defer_gather)
        self.deferred: Dict[int, Deferred] = {}   # id(placeholder) -> its record
        # per-particle scalars broadcast beside a gather placeholder (Normal's broadcast_all of
        # loc and scale): the broadcast view -> the scalar it came from
        self.sources: Dict[int, torch.Tensor] = {}
        self._keep: List[torch.Tensor] = []   # placeholders stay alive: ids are never reused
        self._bypass = False

    # ---- helpers ---------------------------------------------------------------------------
    @contextlib.contextmanager
    def _bypassed(self):
        """Torch calls made inside run as they are (the mode's own calls on real tensors)."""
        previous, self._bypass = self._bypass, True
        try:
            yield
        finally:
            self._bypass = previous

    def lookup(self, tensor: Any, kind: Optional[str] = None) -> Optional[Deferred]:
        """The record of a placeholder (of ``kind``, if given), or None."""
        info = self.deferred.get(id(tensor)) if isinstance(tensor, torch.Tensor) else None
        return info if info is None or kind is None or info.kind == kind else None

    def _accepted(self, tensor: Any, kind: Optional[str], links: Tuple[str, ...]) -> Optional[Deferred]:
        """The record of a placeholder of ``kind`` whose link is one of ``links``, or None."""
        info = self.lookup(tensor, kind)
        return info if info is not None and info.link in links else None

    def _placeholder(self, like: torch.Tensor, info: Deferred) -> torch.Tensor:
        level = _functorch.maybe_get_level(like)
        # never read (any value-reading use materialises the record): no initialising kernel
        device = (info.X if info.kind == "matmul" else info.table).device
        base = torch.empty((), dtype=torch.float32, device=device)
        base = base.expand((self.K,) + tuple(info.shape))
        out = _functorch._add_batch_dim(base, 0, level)
        self.deferred[id(out)] = info
        self._keep.append(out)
        return out

    def _derive(self, src: Any, dst: Any) -> None:
        """``dst`` is a broadcasting view of ``src``: a placeholder if ``src`` is one."""
        info = self.lookup(src)
        if info is None or not isinstance(dst, torch.Tensor):
            return
        shape = torch.Size(dst.shape)
        if info.kind == "matmul":
            derived = _matmul_derived(info.root, shape, info.link, info.steps)
        else:
            derived = info.derived(shape=shape, replay=lambda real: real.expand(shape))
        self.deferred[id(dst)] = derived
        self._keep.append(dst)

    def _real(self, info: Deferred) -> torch.Tensor:
        if info.real is None:
            if info.parent is None:
                _guide.flush_draws()   # theta / the table may be a guide draw not launched yet
                with self._bypassed():
                    info.real = info.replay()
            else:
                real = self._real(info.parent)
                with self._bypassed():
                    info.real = info.replay(real)
        return info.real

    def materialize(self, tensor: torch.Tensor) -> torch.Tensor:
        """
        The real value of a placeholder (computed once), or ``tensor`` itself.
        """
        info = self.lookup(tensor)
        return tensor if info is None else self._real(info)

    def _scalar(self, x: Any) -> bool:
        """A Python number or a per-particle float32 scalar: a term of the affine predictor."""
        if isinstance(x, bool):
            return False
        if isinstance(x, (int, float)):
            return True
        return isinstance(x, torch.Tensor) and _functorch.is_batchedtensor(x) and x.dim() == 0 and \
            x.dtype == torch.float32 and self.lookup(x) is None and lazy_of(x) is None

    # ---- the creation rules ------------------------------------------------------------------
    def _eligible(self, args, kwargs, matrix: bool = False) -> bool:
        """``matrix``: the call is a matmul (not ``mv``), which also takes a [P, C] theta."""
        if kwargs or len(args) != 2:
            return False
        X, theta = args
        if not (isinstance(X, torch.Tensor) and isinstance(theta, torch.Tensor)):
            return False
        if self.lookup(X) is not None or self.lookup(theta) is not None:
            return False   # (the product of a placeholder reads its values)
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
        if self.lookup(table) is not None or lazy_of(table) is not None or \
                lazy_of(index) is not None:
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

    # ---- the derivations: each returns the derived record of a call it accepts, or None --------
    def _exp(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``exp(ph)`` of an identity-link placeholder of either kind: the link "exp"."""
        if func not in _EXPS or len(args) != 1 or kwargs:
            return None
        info = self._accepted(args[0], None, ("identity",))
        if info is None or info.kind == "slope":
            return None
        if info.kind == "matmul":
            return _matmul_derived(info.root, info.shape, "exp")
        return info.derived(link="exp", replay=func)

    def _affine(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``ph + c``, ``ph - c``, ``c - ph`` or ``ph * c`` for an identity-link gather placeholder
        ``ph`` and a scalar ``c``: the same link, with the term composed into shift / mult."""
        op = next((op for op, funcs in _ARITHMETIC.items() if func in funcs), None)
        if op is None or kwargs or len(args) != 2:
            return None
        reflected = _ARITHMETIC[op][func]
        x, y = (args[1], args[0]) if reflected else args   # the call computes x op y
        if self.lookup(x, "gather") is not None and self._scalar(y):
            ph, c, left = x, y, True
        elif self.lookup(y, "gather") is not None and self._scalar(x):
            ph, c, left = y, x, False
        else:
            return None
        info = self._accepted(ph, "gather", ("identity",))
        if info is None:
            return None
        summed = info.X is not None or bool(info.slopes)
        if summed and (op == "mul" or (op == "sub" and not left)):
            return None   # (the kernel's linear term has no factor of its own)
        shift, mult = info.shift, info.mult
        with self._bypassed():   # (per-particle scalars: [K] operations)
            if op == "add":
                shift = c if shift is None else shift + c
            elif op == "sub" and left:
                shift = -c if shift is None else shift - c
            elif op == "sub":
                shift = c if shift is None else c - shift
                mult = -1.0 if mult is None else -mult
            else:
                shift = None if shift is None else shift * c
                mult = c if mult is None else mult * c

        def replay(real):
            operands = (real, c) if left else (c, real)
            return func(*(operands[::-1] if reflected else operands))
        if summed:
            return info.derived(shift=shift, mult=mult, replay=replay,
                                post=info.post + ((op, c, left),),
                                summands=info.summands + ((op, c, left),))
        return info.derived(shift=shift, mult=mult, replay=replay,
                            chain=info.chain + ((op, c, left),))

    def _sum(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``gather + matmul`` in either order (``defer_sum``): an identity-link gather placeholder
        with any affine chain and the identity-link root of ``X @ theta`` for a vector ``theta``,
        both over the same N."""
        if func not in _ADDS or kwargs or len(args) != 2:
            return None
        x, y = (args[1], args[0]) if _ADDS[func] else args   # the call computes x + y
        left = self.lookup(x, "gather") is not None
        g = self._accepted(x if left else y, "gather", ("identity",))
        if g is not None and self.lookup(y if left else x, "slope") is not None:
            return self._sum_slope(func, g, self.lookup(y if left else x, "slope"), left)
        m = self._accepted(y if left else x, "matmul", ("identity",))
        if not self.defer_sum or g is None or m is None or g.X is not None or m.parent is not None or \
                m.theta.dim() != 1 or m.theta.shape[0] > MAX_SUM_FEATURES or \
                tuple(g.shape) != tuple(m.shape) or len(g.shape) != 1 or \
                m.X.device != g.table.device:
            return None

        def replay(real):
            product = self._real(m)
            with self._bypassed():
                operands = (real, product) if left else (product, real)
                return func(*(operands[::-1] if _ADDS[func] else operands))
        return g.derived(X=m.X, theta=m.theta, linear_left=left, replay=replay,
                         summands=g.summands + (("linear", None, left),))

    def _slope(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``gather * z`` in either order (``defer_slope``): a root gather placeholder (identity
        link, no chain, no ``X``, no slopes) and an observed float32 column ``z`` of its length on
        the table's device: a product placeholder."""
        if not self.defer_slope or func not in _MULS or kwargs or len(args) != 2:
            return None
        x, y = (args[1], args[0]) if _MULS[func] else args   # the call computes x * y
        left = self.lookup(x, "gather") is not None
        g = self._accepted(x if left else y, "gather", ("identity",))
        z = y if left else x
        if g is None or g.parent is not None or not isinstance(z, torch.Tensor) or \
                self.lookup(z) is not None or lazy_of(z) is not None or \
                _functorch.is_batchedtensor(z) or z.dtype != torch.float32 or z.dim() != 1 or \
                tuple(z.shape) != tuple(g.shape) or z.device != g.table.device or z.requires_grad:
            return None

        def replay(real):
            operands = (real, z) if left else (z, real)
            return func(*(operands[::-1] if _MULS[func] else operands))
        new = g.derived(replay=replay, z=z, slope_left=left)
        new.kind = "slope"
        return new

    def _sum_slope(self, func: Callable, g: Deferred, p: Deferred, left: bool) -> Optional[Deferred]:
        """``gather + product`` (the gather record the left operand or not): one more slope."""
        if p.parent is None or p.parent.kind != "gather" or p.index is not g.index or \
                len(g.slopes) >= MAX_SLOPES or tuple(g.shape) != tuple(p.shape) or \
                len(g.shape) != 1 or p.table.device != g.table.device:
            return None

        def replay(real):
            product = self._real(p)
            with self._bypassed():
                operands = (real, product) if left else (product, real)
                return func(*(operands[::-1] if _ADDS[func] else operands))
        return g.derived(slopes=g.slopes + ((p.table, p.z, p.slope_left),), replay=replay,
                         summands=g.summands + (("slope", len(g.slopes), left),))

    def _softmax_operand(self, args) -> Optional[Deferred]:
        """The record of ``args[0]`` if a softmax normalisation may derive from it: a [.., N, C]
        placeholder of ``X @ Theta``, raw or normalised already."""
        info = self._accepted(args[0], "matmul", ("identity", "log_softmax")) if args else None
        return info if info is not None and info.theta.dim() == 2 else None

    def _logsumexp(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``logsumexp(ph, -1, keepdim=True)``: the link "logsumexp", [.., N, 1]."""
        info = self._softmax_operand(args) if func in _LOGSUMEXPS else None
        if info is None or not _last_dim(args, kwargs, len(info.shape), {"keepdim": True}):
            return None
        return _matmul_derived(info.root, tuple(info.shape[:-1]) + (1,), "logsumexp", info.steps)

    def _log_softmax(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``log_softmax(ph, -1)``: the link "log_softmax"."""
        info = self._softmax_operand(args) if func in _LOG_SOFTMAXES else None
        if info is None or not (_last_dim(args, kwargs, len(info.shape), {}) or
                                _last_dim(args, kwargs, len(info.shape), {"dtype": None})):
            return None
        return _matmul_derived(info.root, info.shape, "log_softmax", info.steps + ("log_softmax",))

    def _sub_logsumexp(self, func: Callable, args, kwargs) -> Optional[Deferred]:
        """``ph - lse`` for the "logsumexp" placeholder ``lse`` of the same root after the same
        normalisations: the link "log_softmax"."""
        if _SUBS.get(func) is not False or len(args) != 2 or kwargs:
            return None
        info = self._softmax_operand(args)
        other = self._accepted(args[1], "matmul", ("logsumexp",))
        if info is None or other is None or other.root is not info.root or \
                other.steps != info.steps or tuple(other.shape) != tuple(info.shape[:-1]) + (1,):
            return None
        return _matmul_derived(info.root, info.shape, "log_softmax", info.steps + ("sub",))

    # tried in this order; a call none of them accepts materialises its placeholders
    _DERIVATIONS = (_exp, _affine, _slope, _sum, _logsumexp, _log_softmax, _sub_logsumexp)

    # ---- the mode ----------------------------------------------------------------------------
    def __torch_function__(self, func: Callable, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if self._bypass:
            return func(*args, **kwargs)
        if func in _MATMULS and self._eligible(args, kwargs, func not in _MVS):
            X, theta = args
            info = Deferred("matmul", torch.Size((X.shape[0],) + tuple(theta.shape[1:])),
                            X=X, theta=theta, replay=lambda: torch.matmul(X, theta))
            return self._placeholder(theta, info)
        if self.defer_gather and (func in _GETITEMS or func in _INDEX_SELECTS):
            call = self._gather_call(func, args, kwargs)
            if call is not None:
                table, index = call
                info = Deferred("gather", torch.Size(index.shape), table=table, index=index,
                                replay=lambda: func(*args, **kwargs))
                return self._placeholder(table, info)
        if not self.deferred and not _guide._LAZY and \
                (not _guide._PENDING_DRAWS or func in _METADATA or func in _BROADCASTS):
            # no placeholder exists, and no pending draw is read by this call: nothing to do
            return func(*args, **kwargs)
        placeholders = []   # (the tensor, its record)
        lazy = False
        for x in _leaves(args, kwargs):
            info = self.deferred.get(id(x))
            if info is not None:
                placeholders.append((x, info))
            elif lazy_of(x) is not None:
                lazy = True
            elif func not in _METADATA and func not in _BROADCASTS and \
                    _guide.pending_draw(x) is not None:
                # the model reads a guide draw whose launch was left to the loss's planning
                _guide.flush_draws()
        if not placeholders and not lazy:
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
        if not placeholders:
            return func(*args, **kwargs)
        if func in _BROADCASTS:
            out = func(*args, **kwargs)
            if func is torch.broadcast_tensors:
                inputs = args[0] if len(args) == 1 and isinstance(args[0], (list, tuple)) else args
                gathered = any(info.kind == "gather" for _, info in placeholders)
                for src, dst in zip(inputs, list(out)):
                    self._derive(src, dst)
                    if gathered and isinstance(src, torch.Tensor) and src.dim() == 0 and \
                            self.lookup(src) is None:
                        self.sources[id(dst)] = src
                        self._keep.append(dst)
            else:
                self._derive(args[0], out)
            return out
        for derivation in self._DERIVATIONS:
            derived = derivation(self, func, args, kwargs)
            if derived is not None:
                return self._placeholder(placeholders[0][0], derived)
        args, kwargs = tree_map(self.materialize, (args, kwargs))
        return func(*args, **kwargs)


def _summands_back(g, real: torch.Tensor, K: int) -> torch.Tensor:
    """The operations after the gather's chain of a role that holds slopes, in the model's order
    and on its sides: the slope products ``table[:, index] * z``, the product ``X @ theta`` as
    put_back spells a vector regression, the scalar terms."""
    for kind, c, left in g.summands:
        if kind == "slope":
            gathered = g.slope_tables[c][:, g.index]
            term = gathered * g.slope_z[c] if g.slope_left[c] else g.slope_z[c] * gathered
        elif kind == "linear":
            term = g.linear_theta @ g.linear_X.t()
        else:
            term = c.reshape(K, 1) if isinstance(c, torch.Tensor) else c
        if kind == "sub":
            real = real - term
        else:
            real = real + term if left else term + real
    return real


def put_back(site, K: int) -> None:
    """
    Restore what the model wrote where a planner's kernel cannot take a site recorded on a deferred
    predictor (a :class:`mininf_amd.particles.SiteRecord` after the trace, with [K, ...] tensors):
    the predictor becomes the site's own tensor and the record an ordinary site's.
    """
    _guide.flush_draws(claimed=True)
    if site.gather_roles is not None:
        # table[:, index], then the model's own operations in their order (the same elementwise
        # roundings as under vmap), then the link
        for r, g in enumerate(site.gather_roles):
            if g is None:
                continue
            real = g.table[:, g.index]
            for op, c, left in g.chain:
                c = c.reshape(K, 1) if isinstance(c, torch.Tensor) else c
                if op == "add":
                    real = real + c if left else c + real
                elif op == "sub":
                    real = real - c if left else c - real
                else:
                    real = real * c if left else c * real
            if g.slope_tables:
                real = _summands_back(g, real, K)
            elif g.linear_X is not None:
                # the product as put_back spells a vector regression, the sum in the model's
                # operand order, then the later scalar operations
                product = g.linear_theta @ g.linear_X.t()
                real = real + product if g.linear_left else product + real
                for op, c, left in g.post:
                    c = c.reshape(K, 1) if isinstance(c, torch.Tensor) else c
                    if op == "add":
                        real = real + c if left else c + real
                    else:
                        real = real - c
            site.tensors[r] = real.exp() if g.link == "exp" else real
        site.gather_roles = None
        return
    if site.family == "categorical":
        # [K, N, C] logits; the row site normalises them, as Categorical does
        real = torch.matmul(site.linear_X, site.linear_theta)
    else:
        real = site.linear_theta @ site.linear_X.t()   # [K, N]
        if site.linear_link == "exp":
            real = real.exp()
    site.tensors[site.linear_role] = real
    site.linear_X = None
