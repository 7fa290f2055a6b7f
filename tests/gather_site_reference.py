"""
References for mi_gather_site_forward (a Normal / Bernoulli-logits / Poisson site whose parameter is
the gather table[:, index] of a per-particle table [K, G]), shared by test_gather_site_host.py and
test_gpu_gather_site.py.

A case is a dict: family, K, N, G, index [N] (int64, negative entries wrap), roles (two of
("gather", table [K, G], shift, mult, link) | ("particle", q [K]) | ("data", d [N]) |
("constant", c), shift / mult None, a float or [K]), value [N], mask [N] bool or None, site_scale,
g0, strided (tables handed over as [G, K] transposes), null (names of gradients not asked for).

reference():    fp64. With p = table[:, index], eta = shift + mult * p and the role link(eta):
                  Normal    -(v - loc)^2 / (2 s^2) - log s - log sqrt(2 pi)
                  Bernoulli v l - softplus(l)
                  Poisson   v eta - exp(eta) - lgamma(v + 1)            (rate = exp(eta))
                Returns {"total": (value [K], tbound [K]), name: (gradient, bound)} with the names
                role0 / role1 (dtable [K, G] of a gathered role, [K] of a per-particle one),
                shift0 / mult0 / shift1 / mult1 ([K], per-particle terms only). tbound is the sum of
                |site_scale * mask * part| over the rows and the separate parts of the log density,
                bound the sum of the absolute terms of the gradient divided by g0.
float32_restatement(): the kernel's formula in float32 numpy (csrc/gather_site.hip: what a group and
                a particle fix evaluated once, the row's step, fmaf where the kernel has one),
                sums over rows in fp64, a group's parts rounded to float32 where the kernel leaves
                them in its slab (groups that span chunks of ROWS sorted rows).
launch():       one call over poisoned buffers with guard bands around every output.
"""
import ctypes
from math import lgamma as _lgamma

import numpy as np

from mininf_amd import _native as nat

ROWS = nat.GATHER_ROWS
GUARD = 256   # bytes (workspace), elements (outputs)
FAMILIES = {"normal": nat.NORMAL, "bernoulli": nat.BERNOULLI_LOGITS, "poisson": nat.POISSON}
HALF_LOG_2PI = 0.91893853320467274178

lgamma = np.vectorize(_lgamma, otypes=[np.float64])


def wrap(index, G):
    index = np.asarray(index, np.int64)
    return np.where(index < 0, index + G, index)


def sort_plan(index, G):
    """(order, sorted_group) int32, as engine.gather.index_plan."""
    idx = wrap(index, G)
    order = np.argsort(idx, kind="stable")
    return order.astype(np.int32), idx[order].astype(np.int32)


def _term(t, K, default):
    if t is None:
        return np.full(K, default, np.float64)
    return np.broadcast_to(np.asarray(t, np.float64), (K,)).astype(np.float64)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def _names(case):
    """The gradients a launch of the case can write: name -> shape."""
    K, G = case["K"], case["G"]
    out = {}
    for r, role in enumerate(case["roles"]):
        if r == 1 and case["family"] != "normal":
            continue
        if role[0] == "gather":
            out[f"role{r}"] = (K, G)
            if isinstance(role[2], np.ndarray):
                out[f"shift{r}"] = (K,)
            if isinstance(role[3], np.ndarray):
                out[f"mult{r}"] = (K,)
        elif role[0] == "particle":
            out[f"role{r}"] = (K,)
    return out


def reference(case):
    K, N, G = case["K"], case["N"], case["G"]
    idx = wrap(case["index"], G)
    v = np.asarray(case["value"], np.float64)[None, :]
    m = np.ones(N) if case["mask"] is None else np.asarray(case["mask"], np.float64)
    m = m[None, :]
    v = np.where(m != 0, v, 0.0 if case["family"] != "normal" else 0.0)
    scale, g0 = case["site_scale"], case["g0"]
    a, eta, praw = [None, None], [None, None], [None, None]
    for r, role in enumerate(case["roles"]):
        if role[0] == "gather":
            praw[r] = role[1].astype(np.float64)[:, idx]
            eta[r] = _term(role[2], K, 0.0)[:, None] + _term(role[3], K, 1.0)[:, None] * praw[r]
            a[r] = np.exp(eta[r]) if role[4] == "exp" else eta[r]
        elif role[0] == "particle":
            a[r] = np.asarray(role[1], np.float64)[:, None] * np.ones((1, N))
        elif role[0] == "data":
            a[r] = np.asarray(role[1], np.float64)[None, :] * np.ones((K, 1))
        else:
            a[r] = np.full((K, N), float(role[1]))
    family = case["family"]
    with np.errstate(all="ignore"):
        if family == "normal":
            diff = v - a[0]
            parts = [-diff ** 2 / (2 * a[1] ** 2), -np.log(a[1]), np.full((K, N), -HALF_LOG_2PI)]
            d = [diff / a[1] ** 2, (diff ** 2 / a[1] ** 2 - 1) / a[1]]
        elif family == "bernoulli":
            parts = [v * a[0], -np.logaddexp(0.0, a[0])]
            d = [v - _sigmoid(a[0]), None]
        else:
            parts = [v * eta[0], -a[0], -lgamma(np.where(v >= 0, v, 0.0) + 1) * np.ones((K, 1))]
            d = [v / a[0] - 1, None]
    out = {"total": (scale * (m * sum(parts)).sum(1),
                     abs(scale) * (m * sum(np.abs(p) for p in parts)).sum(1))}
    for r, role in enumerate(case["roles"]):
        if d[r] is None:
            continue
        if role[0] == "particle":
            out[f"role{r}"] = (g0 * scale * (m * d[r]).sum(1), abs(scale) * np.abs(m * d[r]).sum(1))
        if role[0] != "gather":
            continue
        deta = m * d[r] * (a[r] if role[4] == "exp" else 1.0)
        mult = _term(role[3], K, 1.0)[:, None]
        onehot = (idx[:, None] == np.arange(G)[None, :]).astype(np.float64)   # [N, G]
        out[f"role{r}"] = (g0 * scale * mult * (deta @ onehot),
                           abs(scale) * np.abs(mult) * (np.abs(deta) @ onehot))
        if isinstance(role[2], np.ndarray):
            out[f"shift{r}"] = (g0 * scale * deta.sum(1), abs(scale) * np.abs(deta).sum(1))
        if isinstance(role[3], np.ndarray):
            out[f"mult{r}"] = (g0 * scale * (deta * praw[r]).sum(1),
                               abs(scale) * np.abs(deta * praw[r]).sum(1))
    return out


def float32_restatement(case):
    """name -> value by the kernel's float32 formula (see the module docstring)."""
    f = np.float32
    K, N, G = case["K"], case["N"], case["G"]
    order, sg = sort_plan(case["index"], G)
    sg = sg.astype(np.int64)
    v = np.asarray(case["value"]).astype(f)[order][None, :]
    m = np.ones(N, bool) if case["mask"] is None else np.asarray(case["mask"], bool)[order]
    scale, g0 = case["site_scale"], case["g0"]
    gscale = float(f(g0)) * scale
    a, eta, praw, chain = [None, None], [None, None], [None, None], [1.0, 1.0]
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f)
    for r, role in enumerate(case["roles"]):
        if role[0] == "gather":
            praw[r] = role[1].astype(f)[:, sg]
            shift = _term(role[2], K, 0.0).astype(f)[:, None]
            mult = _term(role[3], K, 1.0).astype(f)[:, None]
            eta[r] = fma(np.broadcast_to(mult, praw[r].shape), praw[r],
                         np.broadcast_to(shift, praw[r].shape))
            a[r] = eta[r]
            if role[4] == "exp":
                a[r] = np.exp(eta[r]).astype(f)
                if case["family"] != "poisson":
                    chain[r] = a[r]
        elif role[0] == "particle":
            a[r] = np.broadcast_to(np.asarray(role[1], f)[:, None], (K, N))
        elif role[0] == "data":
            a[r] = np.broadcast_to(np.asarray(role[1], f)[order][None, :], (K, N))
        else:
            a[r] = np.full((K, N), f(role[1]))
    family = case["family"]
    rowc = 0.0
    with np.errstate(all="ignore"):
        if family == "normal":
            inv = (f(1) / a[1]).astype(f)
            inv2 = (inv * inv).astype(f)
            c2 = (-(np.log(a[1]).astype(f) + f(HALF_LOG_2PI))).astype(f)
            diff = (v - a[0]).astype(f)
            lp = fma(((f(-0.5) * inv2).astype(f) * diff).astype(f), diff, c2)
            g = (diff * inv2).astype(f)
            d = [g, (fma(diff, g, np.full_like(g, -1)) * inv).astype(f)]
        elif family == "bernoulli":
            t = np.exp(-np.abs(a[0])).astype(f)
            u = (f(1) + t).astype(f)
            c0 = (np.maximum(a[0], f(0)) + np.log1p(t).astype(f)).astype(f)
            sig = np.where(a[0] >= 0, f(1) / u, t / u).astype(f)
            lp = fma(a[0], np.broadcast_to(v, a[0].shape), -c0)
            d = [(v - sig).astype(f), None]
        else:
            lp = fma(np.broadcast_to(v, a[0].shape), eta[0], -a[0])
            d = [(v - a[0]).astype(f), None]
            vv = v[0].astype(np.float64)
            rowc = -(lgamma(np.where(vv >= 0, vv, 0.0) + 1).astype(f).astype(np.float64) * m).sum()
    out = {"total": scale * ((lp.astype(np.float64) * m[None, :]).sum(1) + rowc)}
    starts = np.r_[0, np.flatnonzero(np.diff(sg)) + 1, N]
    for r, role in enumerate(case["roles"]):
        if d[r] is None:
            continue
        if role[0] == "particle":
            out[f"role{r}"] = gscale * (d[r].astype(np.float64) * m[None, :]).sum(1)
        if role[0] != "gather":
            continue
        deta = ((d[r] * chain[r]).astype(f).astype(np.float64)) * m[None, :]
        mult = _term(role[3], K, 1.0).astype(f).astype(np.float64)
        dtable = np.zeros((K, G))
        S_all = np.zeros((K, N))
        for s0, s1 in zip(starts[:-1], starts[1:]):
            c0, c1 = s0 // ROWS, (s1 - 1) // ROWS
            if c0 == c1:
                S = deta[:, s0:s1].sum(1)
            else:   # the chunks' parts pass through float32 (the slab)
                edges = [s0] + [c * ROWS for c in range(c0 + 1, c1 + 1)] + [s1]
                S = sum(deta[:, e0:e1].sum(1).astype(f).astype(np.float64)
                        for e0, e1 in zip(edges[:-1], edges[1:]))
            dtable[:, sg[s0]] = gscale * mult * S
            S_all[:, s0] = deta[:, s0:s1].sum(1)
        out[f"role{r}"] = dtable
        if isinstance(role[2], np.ndarray):
            out[f"shift{r}"] = gscale * S_all.sum(1)
        if isinstance(role[3], np.ndarray):
            out[f"mult{r}"] = gscale * (S_all * praw[r].astype(np.float64)).sum(1)
    return out


def describe(case, tensors, order, sorted_group):
    """The mi_gather_site of a case over ``tensors`` (torch tensors by name, any device)."""
    L = nat.GatherSite()
    L.K, L.N, L.G = case["K"], case["N"], case["G"]
    L.family = FAMILIES[case["family"]]
    for r, role in enumerate(case["roles"]):
        d = L.role[r]
        if role[0] == "gather":
            d.kind = nat.GATHER_GATHER
            d.link = nat.GATHER_LINK_EXP if role[4] == "exp" else nat.GATHER_LINK_IDENTITY
            t = tensors[f"table{r}"]
            d.data = t.data_ptr()
            d.stride_k, d.stride_g = t.stride()
            for name, term in (("shift", role[2]), ("mult", role[3])):
                if isinstance(term, np.ndarray):
                    setattr(d, name + "_kind", nat.GATHER_TERM_PARTICLE)
                    setattr(d, name, tensors[f"{name}{r}"].data_ptr())
                    setattr(d, name + "_stride_k", tensors[f"{name}{r}"].stride(0))
                elif term is not None:
                    setattr(d, name + "_kind", nat.GATHER_TERM_CONSTANT)
                    setattr(d, name + "_constant", float(term))
        elif role[0] == "particle":
            d.kind = nat.GATHER_PARTICLE
            d.data = tensors[f"role{r}"].data_ptr()
            d.stride_k = tensors[f"role{r}"].stride(0)
        elif role[0] == "data":
            d.kind = nat.GATHER_DATA
            d.data = tensors[f"role{r}"].data_ptr()
            d.stride_g = tensors[f"role{r}"].stride(0)
        else:
            d.kind = nat.GATHER_CONSTANT
            d.constant = float(role[1])
    L.order = order.data_ptr()
    L.sorted_group = sorted_group.data_ptr()
    value = tensors["value"]
    L.value = value.data_ptr()
    L.value_stride_i = value.stride(0)
    import torch
    L.value_kind = nat.GATHER_VALUE_INT64 if value.dtype == torch.int64 else nat.GATHER_VALUE_FLOAT32
    if "mask" in tensors:
        L.mask = tensors["mask"].data_ptr()
        L.mask_stride_i = tensors["mask"].stride(0)
    L.grad_scale = case["g0"]
    L.site_scale = case["site_scale"]
    return L


def tensors_of(case, device):
    """The case's operands as torch tensors on ``device`` (tables strided when the case says so)."""
    import torch
    out = {}
    for r, role in enumerate(case["roles"]):
        if role[0] == "gather":
            table = torch.from_numpy(np.ascontiguousarray(role[1], np.float32)).to(device)
            out[f"table{r}"] = table.t().contiguous().t() if case.get("strided") else table
            for name, term in (("shift", role[2]), ("mult", role[3])):
                if isinstance(term, np.ndarray):
                    out[f"{name}{r}"] = torch.from_numpy(term.astype(np.float32)).to(device)
        elif role[0] in ("particle", "data"):
            out[f"role{r}"] = torch.from_numpy(np.asarray(role[1], np.float32)).to(device)
    out["value"] = torch.from_numpy(np.ascontiguousarray(case["value"])).to(device)
    if case["mask"] is not None:
        out["mask"] = torch.from_numpy(np.asarray(case["mask"], bool)).to(device)
    return out


def launch(case, device, sorted_group=None):
    """
    One mi_gather_site_forward of the case over poisoned buffers: (rc, {name: numpy array}, flags).
    ``sorted_group``: a replacement for the plan's (the out-of-range test).
    """
    import torch
    tensors = tensors_of(case, device)
    order, sg = sort_plan(case["index"], case["G"])
    if sorted_group is not None:
        sg = np.asarray(sorted_group, np.int32)
    order_t, sg_t = torch.from_numpy(order).to(device), torch.from_numpy(sg).to(device)
    L = describe(case, tensors, order_t, sg_t)
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_gather_site_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "workspace")
    # O(K N / ROWS): the sums (at most 7 per chunk and particle), the slab (4) and a double per chunk
    chunks = -(-case["N"] // ROWS)
    assert size.value <= chunks * (11 * 4 * case["K"] + 8) + 3 * 256, size.value
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    outs = {"total": torch.full((case["K"] + 2 * GUARD,), float("nan"), device=device)}
    G = nat.GatherGrads()
    for name, shape in _names(case).items():
        if name in case.get("null", ()):
            continue
        buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), float("nan"), device=device)
        outs[name] = buf
        getattr(G, name[:-1])[int(name[-1])] = buf.data_ptr() + 4 * GUARD
    rc = lib.mi_gather_site_forward(ctypes.byref(L), work.data_ptr() + GUARD, size.value,
                                    outs["total"].data_ptr() + 4 * GUARD, ctypes.byref(G),
                                    flags.data_ptr(), nat.stream_handle(device))
    torch.cuda.synchronize()
    assert bool((work[:GUARD] == 0xFF).all()), "the launch wrote below its workspace"
    assert bool((work[GUARD + size.value:] == 0xFF).all()), "the launch wrote past its workspace"
    result = {}
    shapes = dict(_names(case), total=(case["K"],))
    for name, buf in outs.items():
        host = buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all(), \
            f"the launch wrote outside {name}"
        result[name] = host[GUARD:-GUARD].reshape(shapes[name])
    return rc, result, int(flags.cpu()[0]) & 0xFFFFFFFF
