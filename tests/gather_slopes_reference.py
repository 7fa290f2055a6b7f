"""
References for mi_gather_slopes_forward (a group-indexed site whose first role is
shift + mult * table[:, index] + sum_s beta_s[:, index] * z_s + X @ theta), shared by
test_gather_slopes_host.py and test_gpu_gather_slopes_site.py.

A case is a case of tests/gather_linear_reference.py (P may be 0: X [N, 0], theta [K, 0]) with
``slopes``, a list of 1..4 (beta [K, G], z [N]) float32 pairs, and ``z_layout`` (how the columns lie
in memory, see :func:`z_tensors`); ``null`` may name "slope0".."slope3" too, and ``null_slopes``
hands the launch a NULL dslope array.

reference() and float32_restatement() take a case without ``slopes`` as one with none: they are the
references of tests/gather_linear_reference.py too.

reference():    fp64, as gather_site_reference.reference with role 0's eta extended by the slope
                terms and the linear term; "dtheta": (g0 * scale * sum_i m_i * deta0_i * X[i, j], its
                sum of absolute terms divided by g0) and "slope<s>": (g0 * scale * sum_{i in g} m_i *
                deta0_i * z_s[i], likewise), deta0 the per-row quantity that is summed into role 0's
                dtable.
float32_restatement(): the kernel's arithmetic in float32 numpy (csrc/gather_linear_site.hip): eta0
                as fmaf(mult, p, shift), then one fmaf(beta_s, z_s, eta) per slope in order, then
                one fmaf per column of X in order, the row's terms derived per row; dtheta as a
                float sum over each batch of 8 sorted rows folded into a float over the chunk of
                ROWS rows, the chunks' parts added in fp64; dslope as fmaf(de, z, lo) over each
                batch of 8 sorted rows of the chunk, the batches folded into a double per group (a
                group's parts rounded to float32 where the kernel leaves them in its slab);
                everything else as gather_site_reference.float32_restatement.
launch():       one call over poisoned buffers with guard bands around every output.
"""
import ctypes

import numpy as np

from mininf_amd import _native as nat
from tests.gather_linear_reference import (BATCH, _names as _linear_names, describe_linear,
                                           linear_tensors)
from tests.gather_site_reference import (GUARD, HALF_LOG_2PI, ROWS, _sigmoid, _term, describe, lgamma,
                                         sort_plan, wrap)

Z_LAYOUTS = ("plain", "columns", "offset")


def _names(case):
    """The gradients a launch of the case can write: name -> shape."""
    out = dict(_linear_names(case))
    for s in range(len(case["slopes"])):
        out[f"slope{s}"] = (case["K"], case["G"])
    return out


def reference(case):
    K, N, G = case["K"], case["N"], case["G"]
    idx = wrap(case["index"], G)
    v = np.asarray(case["value"], np.float64)[None, :]
    m = np.ones(N) if case["mask"] is None else np.asarray(case["mask"], np.float64)
    m = m[None, :]
    v = np.where(m != 0, v, 0.0)
    scale, g0 = case["site_scale"], case["g0"]
    X = np.asarray(case["X"], np.float64).reshape(N, case["P"])
    X = np.where(m.T != 0, X, 0.0)   # (a masked-out row adds nothing, whatever it holds)
    theta = np.asarray(case["theta"], np.float64).reshape(K, case["P"])
    slopes = case.get("slopes", [])
    zs = [np.where(m[0] != 0, np.asarray(z, np.float64), 0.0) for _, z in slopes]
    a, eta, praw = [None, None], [None, None], [None, None]
    with np.errstate(all="ignore"):
        for r, role in enumerate(case["roles"]):
            if role[0] == "gather":
                praw[r] = role[1].astype(np.float64)[:, idx]
                eta[r] = _term(role[2], K, 0.0)[:, None] + _term(role[3], K, 1.0)[:, None] * praw[r]
                if r == 0:
                    for (beta, _), z in zip(slopes, zs):
                        eta[r] = eta[r] + beta.astype(np.float64)[:, idx] * z[None, :]
                    eta[r] = eta[r] + theta @ X.T
                a[r] = np.exp(eta[r]) if role[4] == "exp" else eta[r]
            elif role[0] == "particle":
                a[r] = np.asarray(role[1], np.float64)[:, None] * np.ones((1, N))
            elif role[0] == "data":
                a[r] = np.asarray(role[1], np.float64)[None, :] * np.ones((K, 1))
            else:
                a[r] = np.full((K, N), float(role[1]))
        family = case["family"]
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
        parts = [np.where(m != 0, p, 0.0) for p in parts]
        out = {"total": (scale * sum(parts).sum(1),
                         abs(scale) * sum(np.abs(p) for p in parts).sum(1))}
        for r, role in enumerate(case["roles"]):
            if d[r] is None:
                continue
            dr = np.where(m != 0, d[r], 0.0)
            if role[0] == "particle":
                out[f"role{r}"] = (g0 * scale * dr.sum(1), abs(scale) * np.abs(dr).sum(1))
            if role[0] != "gather":
                continue
            deta = np.where(m != 0, dr * (a[r] if role[4] == "exp" else 1.0), 0.0)
            mult = _term(role[3], K, 1.0)[:, None]
            onehot = (idx[:, None] == np.arange(G)[None, :]).astype(np.float64)   # [N, G]
            out[f"role{r}"] = (g0 * scale * mult * (deta @ onehot),
                               abs(scale) * np.abs(mult) * (np.abs(deta) @ onehot))
            if isinstance(role[2], np.ndarray):
                out[f"shift{r}"] = (g0 * scale * deta.sum(1), abs(scale) * np.abs(deta).sum(1))
            if isinstance(role[3], np.ndarray):
                out[f"mult{r}"] = (g0 * scale * (deta * praw[r]).sum(1),
                                   abs(scale) * np.abs(deta * praw[r]).sum(1))
            if r == 0:
                out["dtheta"] = (g0 * scale * (deta @ X), abs(scale) * (np.abs(deta) @ np.abs(X)))
                for s, z in enumerate(zs):
                    out[f"slope{s}"] = (g0 * scale * ((deta * z[None, :]) @ onehot),
                                        abs(scale) * (np.abs(deta * z[None, :]) @ onehot))
    return out


def float32_restatement(case):
    """name -> value by the kernel's float32 formula (see the module docstring)."""
    f = np.float32
    K, N, G, P = case["K"], case["N"], case["G"], case["P"]
    order, sg = sort_plan(case["index"], G)
    sg = sg.astype(np.int64)
    v = np.asarray(case["value"]).astype(f)[order][None, :]
    m = np.ones(N, bool) if case["mask"] is None else np.asarray(case["mask"], bool)[order]
    X = np.asarray(case["X"], f).reshape(N, P)[order]          # sorted rows
    theta = np.asarray(case["theta"], f).reshape(K, P)
    slopes = case.get("slopes", [])
    # (a masked-out row reads no z: the kernel holds 0 there)
    zs = [np.where(m, np.asarray(z, f)[order], f(0)) for _, z in slopes]
    scale, g0 = case["site_scale"], case["g0"]
    gscale = float(f(g0)) * scale
    a, eta, praw, chain = [None, None], [None, None], [None, None], [1.0, 1.0]
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f)
    with np.errstate(all="ignore"):
        for r, role in enumerate(case["roles"]):
            if role[0] == "gather":
                praw[r] = role[1].astype(f)[:, sg]
                shift = _term(role[2], K, 0.0).astype(f)[:, None]
                mult = _term(role[3], K, 1.0).astype(f)[:, None]
                eta[r] = fma(np.broadcast_to(mult, praw[r].shape), praw[r],
                             np.broadcast_to(shift, praw[r].shape))
                if r == 0:
                    for (beta, _), z in zip(slopes, zs):   # one fmaf per slope, in order
                        eta[r] = fma(beta.astype(f)[:, sg], np.broadcast_to(z[None, :], eta[r].shape),
                                     eta[r])
                    for j in range(P):   # one fmaf per column, in order
                        eta[r] = fma(np.broadcast_to(X[None, :, j], eta[r].shape),
                                     np.broadcast_to(theta[:, j:j + 1], eta[r].shape), eta[r])
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
        lp = np.where(m[None, :], lp.astype(np.float64), 0.0)
    out = {"total": scale * (lp.sum(1) + rowc)}
    starts = np.r_[0, np.flatnonzero(np.diff(sg)) + 1, N]

    def group_sums(term, factor):
        """[K, G]: factor * a group's sum of term [K, N] (fp64 values), its chunks' parts through
        float32 where the group spans chunks; and the groups' sums at their first rows [K, N]."""
        table = np.zeros((K, G))
        first = np.zeros((K, N))
        for s0, s1 in zip(starts[:-1], starts[1:]):
            c0, c1 = s0 // ROWS, (s1 - 1) // ROWS
            if c0 == c1:
                S = term[:, s0:s1].sum(1)
            else:   # the chunks' parts pass through float32 (the slab)
                edges = [s0] + [c * ROWS for c in range(c0 + 1, c1 + 1)] + [s1]
                S = sum(term[:, e0:e1].sum(1).astype(f).astype(np.float64)
                        for e0, e1 in zip(edges[:-1], edges[1:]))
            table[:, sg[s0]] = factor * S
            first[:, s0] = term[:, s0:s1].sum(1)
        return table, first

    for r, role in enumerate(case["roles"]):
        if d[r] is None:
            continue
        if role[0] == "particle":
            out[f"role{r}"] = gscale * np.where(m[None, :], d[r].astype(np.float64), 0.0).sum(1)
        if role[0] != "gather":
            continue
        de32 = (d[r] * chain[r]).astype(f)
        deta = np.where(m[None, :], de32.astype(np.float64), 0.0)
        mult = _term(role[3], K, 1.0).astype(f).astype(np.float64)
        out[f"role{r}"], S_all = group_sums(deta, gscale * mult)
        if isinstance(role[2], np.ndarray):
            out[f"shift{r}"] = gscale * S_all.sum(1)
        if isinstance(role[3], np.ndarray):
            out[f"mult{r}"] = gscale * (S_all * praw[r].astype(np.float64)).sum(1)
        if r != 0:
            continue
        # dtheta: a float over a batch of BATCH rows, folded into a float over the chunk, the
        # chunks in fp64
        dtheta = np.zeros((K, P))
        # dslope: fmaf(de, z, lo) over the observed rows of a batch (lo restarts with the batch; a
        # group that ends inside a batch takes lo as it stands), the batches' values in fp64
        part = [np.zeros((K, N)) for _ in zs]   # what each row's step added to its group's double
        for c0 in range(0, N, ROWS):
            hi = np.zeros((K, P), f)
            for b0 in range(c0, min(N, c0 + ROWS), BATCH):
                lo = np.zeros((K, P), f)
                los = [np.zeros(K, f) for _ in zs]
                rows = range(b0, min(N, c0 + ROWS, b0 + BATCH))
                for i in rows:
                    if i > b0 and sg[i] != sg[i - 1]:
                        # the group ended: take() read hi + lo, the next group starts at 0
                        for s in range(len(zs)):
                            part[s][:, i - 1] += los[s].astype(np.float64)
                            los[s] = np.zeros(K, f)
                    if m[i]:
                        lo = fma(np.broadcast_to(de32[:, i:i + 1], lo.shape),
                                 np.broadcast_to(X[i][None, :], lo.shape), lo)
                        for s, z in enumerate(zs):
                            los[s] = fma(de32[:, i], np.broadcast_to(z[i], (K,)), los[s])
                for s in range(len(zs)):   # the fold at the batch's end
                    part[s][:, rows[-1]] += los[s].astype(np.float64)
                hi = (hi + lo).astype(f)
            dtheta += hi.astype(np.float64)
        out["dtheta"] = gscale * dtheta
        for s in range(len(zs)):
            out[f"slope{s}"], _ = group_sums(part[s], gscale)
    return out


def z_tensors(case, device):
    """The columns z_s on ``device`` as ``z_layout`` says: "plain" one contiguous tensor each;
    "columns" the strided columns of one [N, S] matrix; "offset" contiguous, one float past an
    aligned address."""
    import torch
    zs = [torch.from_numpy(np.ascontiguousarray(z, np.float32)) for _, z in case["slopes"]]
    layout = case.get("z_layout", "plain")
    if layout == "columns":
        matrix = torch.stack(zs, 1).contiguous().to(device)
        return [matrix[:, s] for s in range(len(zs))]
    if layout == "offset":
        out = []
        for z in zs:
            flat = torch.full((z.numel() + 1,), float("nan"))
            flat[1:] = z
            out.append(flat.to(device)[1:])
        return out
    return [z.to(device) for z in zs]


def slopes_tensors(case, device):
    import torch
    tensors = linear_tensors(case, device)
    for s, (beta, _) in enumerate(case["slopes"]):
        table = torch.from_numpy(np.ascontiguousarray(beta, np.float32)).to(device)
        tensors[f"beta{s}"] = table.t().contiguous().t() if case.get("strided") else table
    for s, z in enumerate(z_tensors(case, device)):
        tensors[f"z{s}"] = z
    return tensors


def describe_slopes(case, tensors, order, sorted_group):
    """The mi_gather_slopes of a case over ``tensors``."""
    M = nat.GatherSlopes()
    if case["P"] > 0:
        M.linear = describe_linear(case, tensors, order, sorted_group)
    else:   # x and theta stay NULL
        M.linear.site = describe(case, tensors, order, sorted_group)
    M.S = len(case["slopes"])
    for s in range(len(case["slopes"])):
        table, z = tensors[f"beta{s}"], tensors[f"z{s}"]
        M.slope[s].table = table.data_ptr()
        M.slope[s].stride_k, M.slope[s].stride_g = table.stride()
        M.slope[s].z = z.data_ptr()
        M.slope[s].z_stride_i = z.stride(0)
    return M


def launch(case, device):
    """
    One mi_gather_slopes_forward of the case over poisoned buffers: (rc, {name: numpy array}, flags).
    """
    import torch
    tensors = slopes_tensors(case, device)
    order, sg = sort_plan(case["index"], case["G"])
    order_t, sg_t = torch.from_numpy(order).to(device), torch.from_numpy(sg).to(device)
    M = describe_slopes(case, tensors, order_t, sg_t)
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_gather_slopes_workspace_bytes(ctypes.byref(M), ctypes.byref(size)), "workspace")
    # mi_gather_linear's O(K N / ROWS) and 2 K S floats per chunk
    chunks = -(-case["N"] // ROWS)
    S = len(case["slopes"])
    assert size.value <= chunks * ((11 + case["P"] + 2 * S) * 4 * case["K"] + 8) + 5 * 256, size.value
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    outs = {"total": torch.full((case["K"] + 2 * GUARD,), float("nan"), device=device)}
    G = nat.GatherGrads()
    dtheta = None
    dslope = (nat.c_vp * nat.GATHER_MAX_SLOPES)()
    for name, shape in _names(case).items():
        if name in case.get("null", ()) or (name.startswith("slope") and case.get("null_slopes")):
            continue
        buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), float("nan"), device=device)
        outs[name] = buf
        if name == "dtheta":
            dtheta = buf.data_ptr() + 4 * GUARD
        elif name.startswith("slope"):
            dslope[int(name[5:])] = buf.data_ptr() + 4 * GUARD
        else:
            getattr(G, name[:-1])[int(name[-1])] = buf.data_ptr() + 4 * GUARD
    rc = lib.mi_gather_slopes_forward(ctypes.byref(M), work.data_ptr() + GUARD, size.value,
                                      outs["total"].data_ptr() + 4 * GUARD, ctypes.byref(G), dtheta,
                                      None if case.get("null_slopes") else dslope,
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
