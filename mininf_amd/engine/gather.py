"""
Group-indexed sites: Normal / Bernoulli-logits / Poisson sites whose parameter is the model's own
gather ``alpha[group]`` of a per-particle table [K, G], fused (``mi_gather_site_forward``; the
gather was deferred by :mod:`mininf_amd.linear`), and those whose first role also has fixed
effects, ``alpha[group] + X @ theta`` (``mi_gather_linear_forward``: theta [K, P] joins the
launcher's parameters) or varying slopes, ``alpha[group] + beta[group] * z [+ X @ theta]``
(``mi_gather_slopes_forward``: the slope tables [K, G] join the parameters too). Such a site is
planned as a row site -- an entry (site, parameters, value, mask) of the planner's categorical list
whose record carries its launcher (``site.launcher``, run by ``engine._rows._run_row_site`` under
the row sites' one contract) -- so the ELBO plan, ``log_joint`` and ``LogLikelihoodLoss`` take it
like any row site: its speculative gradients are dense in every parameter (the tables [K, G],
per-particle roles, shifts and mults [K]), and it declines absorption like every row site.

The kernel reads the rows sorted by group: :func:`index_plan` turns the model's index into
(order, sorted_group) once per index tensor.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Dict, List, Optional, Tuple

import torch

from .. import _native as nat
from .. import data
from ..linear import put_back as _materialise   # (the gather back as the model wrote it)
from ..particles import SiteRecord
from ._operands import FAMILY_CODES, _collapse, _to_device
from ._rows import _buffers

# Index plans by (data pointer, shape, stride, dtype, device, G): (weakref to the index, its
# version, (order, sorted_group) or None for an index out of range). The sort and the range
# check's host synchronisation happen once per index tensor, not every step.
_PLANS: Dict[Tuple, Tuple[weakref.ref, int, Optional[Tuple[torch.Tensor, torch.Tensor]]]] = {}
_MAX_PLANS = 64


def index_plan(index: torch.Tensor, G: int) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """
    (order, sorted_group), both int32 [N], of an unbatched 1-D integer ``index`` into G groups:
    ``order`` the rows stable-sorted by group (negative indices wrapped as torch wraps them),
    ``sorted_group[j] = index[order[j]]``. None for an index out of range (remembered:
    :func:`out_of_range` then says so and ``plan_gather`` raises ``IndexError`` on the host,
    where torch's own gather would fail an assertion on the device), and -- the caller then
    materialises the gather as the model wrote it -- for a plan first needed while the stream is
    capturing and for a minibatch column of a ``DeviceDataLoader`` (its values change every step).
    """
    if index.dim() != 1 or index.dtype not in (torch.int64, torch.int32) or \
            not 0 < index.shape[0] < 2 ** 31 or data.lookup(index) is not None:
        return None
    key = (index.data_ptr(), tuple(index.shape), tuple(index.stride()), index.dtype,
           str(index.device), int(G))
    hit = _PLANS.get(key)
    if hit is not None and hit[0]() is index and hit[1] == index._version:
        return hit[2]
    if index.is_cuda and torch.cuda.is_current_stream_capturing():
        return None   # (the range check reads the index on the host)
    with torch.no_grad():
        wrapped = index.to(torch.int64)
        wrapped = torch.where(wrapped < 0, wrapped + G, wrapped)
        plan = None
        if not bool(((wrapped < 0) | (wrapped >= G)).any()):
            sorted_group, order = torch.sort(wrapped, stable=True)
            plan = (order.to(torch.int32), sorted_group.to(torch.int32))
    _PLANS[key] = (weakref.ref(index), index._version, plan)
    while len(_PLANS) > _MAX_PLANS:
        _PLANS.pop(next(iter(_PLANS)))
    return plan


def out_of_range(index: torch.Tensor, G: int) -> bool:
    """Whether :func:`index_plan` found ``index`` (this version of it) outside [-G, G)."""
    key = (index.data_ptr(), tuple(index.shape), tuple(index.stride()), index.dtype,
           str(index.device), int(G))
    hit = _PLANS.get(key)
    return hit is not None and hit[0]() is index and hit[1] == index._version and hit[2] is None


class _Role:
    """One parameter role of the launch: its kind, the tensor read and the affine terms."""
    def __init__(self, kind: int) -> None:
        self.kind = kind
        self.link = nat.GATHER_LINK_IDENTITY
        self.tensor: Optional[torch.Tensor] = None   # GATHER [K, G], PARTICLE [K, 1], DATA [N]
        self.constant = 0.0
        self.shift = None    # None, a float or a [K] tensor
        self.mult = None
        # positions among the launcher's parameters (autograd inputs), or -1
        self.param = self.shift_param = self.mult_param = -1
        # role 0's linear term: the observed X [N, P] and theta's position among the parameters
        self.X: Optional[torch.Tensor] = None
        self.theta_param = -1
        # role 0's slope terms: the observed columns [N] and the tables' positions
        self.slope_z: List[torch.Tensor] = []
        self.slope_params: List[int] = []


class _GatherLauncher:
    """One ``mi_gather_site_forward`` / ``mi_gather_linear_forward`` / ``mi_gather_slopes_forward``
    site."""
    def __init__(self, site: SiteRecord, K: int, device: torch.device, roles: List[_Role],
                 order: torch.Tensor, sorted_group: torch.Tensor, G: int, value: torch.Tensor,
                 mask: Optional[torch.Tensor]) -> None:
        self.site, self.K, self.device = site, K, device
        self.roles = roles
        self.order, self.sorted_group = order, sorted_group
        self.N, self.G = int(order.shape[0]), G
        self.value = value            # [N] float32 or int64
        self.mask = mask              # [N] bool or None
        self.launches = 0             # kernel calls that ran (not declined)
        self.linear = roles[0].X is not None   # an X @ theta term (mi_gather_linear_forward)
        self.slopes = bool(roles[0].slope_params)   # mi_gather_slopes_forward

    def describe(self, params: Tuple[torch.Tensor, ...], g0: float, grad_ptr):
        """
        The launch's descriptor: (the outermost struct, the ``nat.GatherSite`` inside it, the stem
        of the library's entry points for it, the forward's arguments after the role gradients).
        ``grad_ptr(where)``: the address of ``params[where]``'s gradient, or None.
        """
        role = self.roles[0]
        if not self.linear and not self.slopes:
            L = nat.GatherSite()
            self._describe_site(L, params, g0)
            return L, L, "mi_gather_site", ()
        M = nat.GatherSlopes() if self.slopes else nat.GatherLinear()
        linear = M.linear if self.slopes else M   # (P = 0 where the slopes have no X @ theta)
        site = linear.site
        self._describe_site(site, params, g0)
        dtheta = None
        if self.linear:
            X, theta = role.X, params[role.theta_param]
            linear.P = int(X.shape[1])
            linear.x = X.data_ptr()
            linear.x_stride_i, linear.x_stride_j = X.stride()
            linear.theta = theta.data_ptr()
            linear.theta_stride_k, linear.theta_stride_j = theta.stride()
            dtheta = grad_ptr(role.theta_param)   # [K, P] contiguous, every entry written
        if not self.slopes:
            return M, site, "mi_gather_linear", (dtheta,)
        M.S = len(role.slope_params)
        dslope = (nat.c_vp * nat.GATHER_MAX_SLOPES)()
        for s, (where, z) in enumerate(zip(role.slope_params, role.slope_z)):
            table = params[where]
            M.slope[s].table = table.data_ptr()
            M.slope[s].stride_k, M.slope[s].stride_g = table.stride()
            M.slope[s].z = z.data_ptr()
            M.slope[s].z_stride_i = z.stride(0)
            dslope[s] = grad_ptr(where)   # [K, G] contiguous, every entry written
        return M, site, "mi_gather_slopes", (dtheta, dslope)

    def _describe_site(self, L: nat.GatherSite, params: Tuple[torch.Tensor, ...],
                       g0: float) -> None:
        """Fill ``L``, the site without its linear and slope terms."""
        L.K, L.N, L.G = self.K, self.N, self.G
        L.family = FAMILY_CODES[self.site.family]
        for r, role in enumerate(self.roles):
            d = L.role[r]
            d.kind, d.link = role.kind, role.link
            tensor = params[role.param] if role.param >= 0 else role.tensor
            if role.kind == nat.GATHER_GATHER:
                d.data = tensor.data_ptr()
                d.stride_k, d.stride_g = tensor.stride()
            elif role.kind == nat.GATHER_PARTICLE:
                d.data = tensor.data_ptr()
                d.stride_k = tensor.stride(0)
            elif role.kind == nat.GATHER_DATA:
                d.data = tensor.data_ptr()
                d.stride_g = tensor.stride(0)
            else:
                d.constant = role.constant
            for name, term, where in (("shift", role.shift, role.shift_param),
                                      ("mult", role.mult, role.mult_param)):
                if term is None:
                    continue
                if isinstance(term, torch.Tensor):
                    t = params[where] if where >= 0 else term
                    setattr(d, name + "_kind", nat.GATHER_TERM_PARTICLE)
                    setattr(d, name, t.data_ptr())
                    setattr(d, name + "_stride_k", t.stride(0))
                else:
                    setattr(d, name + "_kind", nat.GATHER_TERM_CONSTANT)
                    setattr(d, name + "_constant", float(term))
        L.order = self.order.data_ptr()
        L.sorted_group = self.sorted_group.data_ptr()
        L.value = self.value.data_ptr()
        L.value_stride_i = self.value.stride(0)
        L.value_kind = nat.GATHER_VALUE_INT64 if self.value.dtype == torch.int64 \
            else nat.GATHER_VALUE_FLOAT32
        if self.mask is not None:
            L.mask = self.mask.data_ptr()
            L.mask_stride_i = self.mask.stride(0)
        L.grad_scale = g0
        L.site_scale = self.site.scale

    def run(self, params: Tuple[torch.Tensor, ...], g0: float,
            flags: Optional[torch.Tensor] = None):
        """(total [K], the speculative gradients of ``params`` -- None where none is needed --,
        no dvalue, flags [1])."""
        device = self.device
        grads: List[Optional[torch.Tensor]] = [None] * len(params)

        def grad_ptr(where: int) -> Optional[int]:
            if where < 0 or not params[where].requires_grad:
                return None
            # (every entry written; a per-particle parameter's in its own shape)
            grads[where] = torch.empty(tuple(params[where].shape), dtype=torch.float32,
                                       device=device)
            return grads[where].data_ptr()

        G = nat.GatherGrads()
        for r, role in enumerate(self.roles):
            G.role[r] = grad_ptr(role.param)
            G.shift[r] = grad_ptr(role.shift_param)
            G.mult[r] = grad_ptr(role.mult_param)
        L, site, stem, extra = self.describe(params, g0, grad_ptr)
        if flags is not None:
            site.options |= nat.GROUP_FLAGS_ZEROED
        size = ctypes.c_size_t()
        lib = nat.lib()
        code = getattr(lib, stem + "_workspace_bytes")(ctypes.byref(L), ctypes.byref(size))
        # (only the linear and slopes queries decline a site; the plain one's codes are all errors)
        if code == nat.MI_EUNSUPPORTED and stem != "mi_gather_site":
            return self._materialised(params, g0, flags)
        nat.check(code, stem + "_workspace_bytes")
        workspace, total, words = _buffers(size.value, self.K, device, flags)
        code = getattr(lib, stem + "_forward")(
            ctypes.byref(L), workspace.data_ptr(), size.value, total.data_ptr(), ctypes.byref(G),
            *extra, words.data_ptr(), nat.stream_handle(device))
        if code == nat.MI_EUNSUPPORTED:
            return self._materialised(params, g0, flags)
        nat.check(code, stem + "_forward")
        self.launches += 1
        return total, tuple(grads), None, words

    def _predictor(self, r: int, params: Tuple[torch.Tensor, ...]) -> torch.Tensor:
        """Role r as the model would have computed it: [K, N] (or a broadcastable view)."""
        role = self.roles[r]
        tensor = params[role.param] if role.param >= 0 else role.tensor
        if role.kind == nat.GATHER_CONSTANT:
            return torch.full((1, 1), role.constant, device=self.device)
        if role.kind == nat.GATHER_PARTICLE:
            return tensor.reshape(self.K, 1)
        if role.kind == nat.GATHER_DATA:
            return tensor.reshape(1, self.N)
        index = torch.empty(self.N, dtype=torch.int64, device=self.device)
        index[self.order.long()] = self.sorted_group.long()
        linear = params[role.theta_param] @ role.X.t() if role.X is not None else None
        for where, z in zip(role.slope_params, role.slope_z):
            term = params[where][:, index] * z
            linear = term if linear is None else linear + term
        return _affine(tensor[:, index], params[role.shift_param] if role.shift_param >= 0
                       else role.shift, params[role.mult_param] if role.mult_param >= 0
                       else role.mult, role.link == nat.GATHER_LINK_EXP, linear)

    def _materialised(self, params: Tuple[torch.Tensor, ...], g0: float,
                      flags: Optional[torch.Tensor]):
        """The launch the library declined, through torch on the materialised gather: what
        :meth:`run` returns (torch validates nothing here: with no ``flags`` given, a zero word)."""
        from torch.distributions import Bernoulli, Normal, Poisson
        if flags is None:
            flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        leaves = [p.detach().requires_grad_(p.requires_grad) for p in params]
        with torch.enable_grad():
            a = [self._predictor(r, tuple(leaves)) for r in range(2)]
            value = self.value.to(torch.float32).reshape(1, self.N)
            family = self.site.family
            dist = Normal(a[0], a[1], validate_args=False) if family == "normal" else \
                Bernoulli(logits=a[0], validate_args=False) if family == "bernoulli_logits" else \
                Poisson(a[0], validate_args=False)
            lp = dist.log_prob(value)
            if self.mask is not None:
                lp = torch.where(self.mask.reshape(1, self.N), lp, torch.zeros_like(lp))
            total = lp.expand(self.K, self.N).sum(1) * self.site.scale
            wanted = [p for p in leaves if p.requires_grad]
            got = iter(torch.autograd.grad(total.sum() * g0, wanted, allow_unused=True)
                       if wanted else ())
        grads = tuple((next(got) if p.requires_grad else None) for p in leaves)
        grads = tuple(torch.zeros_like(p) if g is None and p.requires_grad else g
                      for g, p in zip(grads, leaves))
        return total.detach(), grads, None, flags


def _affine(gathered: torch.Tensor, shift, mult, exp: bool, linear=None) -> torch.Tensor:
    """link(shift + mult * gathered [+ linear]) for [K, N] ``gathered`` (and ``linear``, the slope
    terms and the fixed effects together) and None / number / [K] terms."""
    K = gathered.shape[0]
    if mult is not None:
        gathered = (mult.reshape(K, 1) if isinstance(mult, torch.Tensor) else mult) * gathered
    if shift is not None:
        gathered = (shift.reshape(K, 1) if isinstance(shift, torch.Tensor) else shift) + gathered
    if linear is not None:
        gathered = gathered + linear
    return gathered.exp() if exp else gathered


def plan_gather(site: SiteRecord, K: int, device: torch.device):
    """
    The row-site entry (site, parameters, value, mask) of a site recorded on a deferred gather, or
    None after materialising the gather as the model would have written it (``table[:, index]``,
    [K, N]) where the kernel cannot take the operands or the index has no plan: the site is then
    grouped like any other.
    """
    shape = site.site_shape
    N = int(shape.numel())
    live = [g for g in site.gather_roles if g is not None]
    index = live[0].index
    ok = len(shape) == 1 and index.device == device and all(
        g.table.dtype == torch.float32 and g.table.dim() == 2 and g.table.device == device and
        all(not isinstance(t, torch.Tensor) or (t.dtype == torch.float32 and t.device == device and
                                                t.numel() == K)
            for t in (g.shift, g.mult)) for g in live)
    # a linear term: float32 X [N, P] and theta [K, P] on the device, X held whole (not a
    # DeviceDataLoader column), P within the kernel's registers
    for g in live:
        if g.linear_X is not None:
            X, theta = g.linear_X, g.linear_theta
            ok = ok and g is site.gather_roles[0] and len(live) == 1 and \
                X.dtype == torch.float32 and X.device == device and not X.requires_grad and \
                X.dim() == 2 and X.shape[0] == N and \
                1 <= X.shape[1] <= nat.GATHER_LINEAR_MAX_P and data.lookup(X) is None and \
                theta.dtype == torch.float32 and theta.device == device and \
                tuple(theta.shape) == (K, X.shape[1])
        if g.slope_tables:
            # slope terms: float32 tables [K, G'] (G' = G is checked below) and float32 columns
            # [N] on the device, held whole (not a DeviceDataLoader column)
            ok = ok and g is site.gather_roles[0] and len(live) == 1 and \
                len(g.slope_tables) <= nat.GATHER_MAX_SLOPES and all(
                    t.dtype == torch.float32 and t.dim() == 2 and t.device == device and
                    t.shape[0] == K and
                    z.dtype == torch.float32 and z.device == device and not z.requires_grad and
                    z.dim() == 1 and z.shape[0] == N and data.lookup(z) is None
                    for t, z in zip(g.slope_tables, g.slope_z))
    G = int(live[0].table.shape[1]) if ok else 0
    ok = ok and all(int(t.shape[1]) == G for g in live for t in [g.table, *g.slope_tables])
    ok_index = ok
    plan = index_plan(index, G) if ok else None
    roles: List[_Role] = []
    params: List[torch.Tensor] = []
    if plan is not None:
        value_t, _ = _to_device(site.tensors[-1], K, device, f"site '{site.name}'",
                                allow_constant=False)
        view = _collapse(value_t, K, shape)
        # (one particle -- LogLikelihoodLoss -- has no particle axis to depend on)
        ok = (view.sk == 0 or K == 1) and value_t.dtype in (torch.int64, torch.float32) and \
            not value_t.requires_grad
    else:
        ok = False
    for r, g in enumerate(site.gather_roles if ok else ()):
        if g is not None:
            role = _Role(nat.GATHER_GATHER)
            role.link = nat.GATHER_LINK_EXP if g.link == "exp" else nat.GATHER_LINK_IDENTITY
            role.param = len(params)
            params.append(g.table)
            for name, term in (("shift", g.shift), ("mult", g.mult)):
                if isinstance(term, torch.Tensor):
                    setattr(role, name + "_param", len(params))
                    params.append(term.reshape(K))
                setattr(role, name, term)
            if g.linear_X is not None:
                role.X = g.linear_X
                role.theta_param = len(params)
                params.append(g.linear_theta)
            for table, z in zip(g.slope_tables, g.slope_z):
                role.slope_params.append(len(params))
                params.append(table)
                role.slope_z.append(z)
            roles.append(role)
            continue
        t, constant = _to_device(site.tensors[r], K, device, f"site '{site.name}'")
        if constant is not None:
            role = _Role(nat.GATHER_CONSTANT)
            role.constant = constant
        elif t.dtype != torch.float32:
            ok = False
            break
        else:
            v = _collapse(t, K, shape)
            if v.si == 0 or N == 1:
                role = _Role(nat.GATHER_PARTICLE)
                # one scalar per particle, in the tensor's own shape when it has K elements
                role.tensor = t if t.numel() == K else v.tensor[:, :1]
                role.param = len(params)
                params.append(role.tensor)
            elif v.sk == 0 and not t.requires_grad:
                role = _Role(nat.GATHER_DATA)
                role.tensor = v.tensor[0]
            else:
                ok = False
                break
        roles.append(role)
    if ok:
        while len(roles) < 2:
            roles.append(_Role(nat.GATHER_CONSTANT))
        value = view.tensor[0]
        mask = None
        if site.mask is not None:
            mask = site.mask.to(device).bool().expand(shape).reshape(-1)
        site.launcher = _GatherLauncher(site, K, device, roles, plan[0], plan[1], G, value, mask)
        return site, tuple(params), value, mask
    if ok_index and out_of_range(index, G):
        # (torch's own gather would raise this on the host and fail an assertion on the device)
        raise IndexError(f"site '{site.name}': index out of range in the group index of a table "
                         f"with {G} groups")
    _materialise(site, K)
    return None
