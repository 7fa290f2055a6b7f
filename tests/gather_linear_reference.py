"""
References for mi_gather_linear_forward (a group-indexed site whose first role is
shift + mult * table[:, index] + X @ theta), shared by test_gather_linear_host.py and
test_gpu_gather_linear_site.py.

A case is a case of tests/gather_site_reference.py (role 0 gathered) with X [N, P] and theta [K, P]
(float32), ``x_layout`` (how X lies in memory, see :func:`x_tensor`) and ``theta_strided``; ``null``
may name "dtheta" too.

reference() and float32_restatement() are those of tests/gather_slopes_reference.py (one kernel,
csrc/gather_linear_site.hip, evaluates both sites) for a case without slopes:
reference():    fp64, with "dtheta": (g0 * scale * sum_i m_i * deta0_i * X[i, j], its sum of absolute
                terms divided by g0), deta0 the per-row quantity that is summed into role 0's dtable.
float32_restatement(): the kernel's arithmetic in float32 numpy.
launch():       one call over poisoned buffers with guard bands around every output.
"""
import ctypes

import numpy as np

from mininf_amd import _native as nat
from tests.gather_site_reference import (GUARD, ROWS, _names as _site_names, describe, sort_plan,
                                         tensors_of)

BATCH = 8   # kGsBatch: rows per fold of the float sums
X_LAYOUTS = ("plain", "slice", "slice1", "offset", "transposed")


def _names(case):
    """The gradients a launch of the case can write: name -> shape."""
    out = dict(_site_names(case))
    out["dtheta"] = (case["K"], case["P"])
    return out


def reference(case):
    from tests.gather_slopes_reference import reference as with_slopes   # (it imports this module)
    return with_slopes(case)


def float32_restatement(case):
    """name -> value by the kernel's float32 formula (see the module docstring)."""
    from tests.gather_slopes_reference import float32_restatement as with_slopes
    return with_slopes(case)


def x_tensor(case, device):
    """X of the case on ``device`` as its ``x_layout`` says: "plain" contiguous; "slice" the first
    P columns of a wider matrix whose rows stay 16-byte aligned; "slice1" P columns from the second
    on; "offset" contiguous, one float past an aligned address; "transposed" [P, N] memory."""
    import torch
    X = torch.from_numpy(np.ascontiguousarray(case["X"], np.float32))
    N, P = X.shape
    layout = case.get("x_layout", "plain")
    if layout == "plain":
        return X.to(device)
    if layout in ("slice", "slice1"):
        wide = torch.full((N, (P + 3) // 4 * 4 + 4), float("nan"))
        first = 1 if layout == "slice1" else 0
        wide[:, first:first + P] = X
        return wide.to(device)[:, first:first + P]
    if layout == "offset":
        flat = torch.full((N * P + 1,), float("nan"))
        flat[1:] = X.reshape(-1)
        return flat.to(device)[1:].view(N, P)
    return X.t().contiguous().to(device).t()


def theta_tensor(case, device):
    import torch
    theta = torch.from_numpy(np.ascontiguousarray(case["theta"], np.float32)).to(device)
    return theta.t().contiguous().t() if case.get("theta_strided") else theta


def describe_linear(case, tensors, order, sorted_group):
    """The mi_gather_linear of a case over ``tensors`` (with "X" and "theta" among them)."""
    L = nat.GatherLinear()
    L.site = describe(case, tensors, order, sorted_group)
    L.P = case["P"]
    X, theta = tensors["X"], tensors["theta"]
    L.x = X.data_ptr()
    L.x_stride_i, L.x_stride_j = X.stride()
    L.theta = theta.data_ptr()
    L.theta_stride_k, L.theta_stride_j = theta.stride()
    return L


def linear_tensors(case, device):
    tensors = tensors_of(case, device)
    tensors["X"] = x_tensor(case, device)
    tensors["theta"] = theta_tensor(case, device)
    return tensors


def launch(case, device, sorted_group=None):
    """
    One mi_gather_linear_forward of the case over poisoned buffers: (rc, {name: numpy array}, flags).
    """
    import torch
    tensors = linear_tensors(case, device)
    order, sg = sort_plan(case["index"], case["G"])
    if sorted_group is not None:
        sg = np.asarray(sorted_group, np.int32)
    order_t, sg_t = torch.from_numpy(order).to(device), torch.from_numpy(sg).to(device)
    L = describe_linear(case, tensors, order_t, sg_t)
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_gather_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "workspace")
    # mi_gather_site's O(K N / ROWS) and K P floats per chunk
    chunks = -(-case["N"] // ROWS)
    assert size.value <= chunks * ((11 + case["P"]) * 4 * case["K"] + 8) + 4 * 256, size.value
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    outs = {"total": torch.full((case["K"] + 2 * GUARD,), float("nan"), device=device)}
    G = nat.GatherGrads()
    dtheta = None
    for name, shape in _names(case).items():
        if name in case.get("null", ()):
            continue
        buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), float("nan"), device=device)
        outs[name] = buf
        if name == "dtheta":
            dtheta = buf.data_ptr() + 4 * GUARD
        else:
            getattr(G, name[:-1])[int(name[-1])] = buf.data_ptr() + 4 * GUARD
    rc = lib.mi_gather_linear_forward(ctypes.byref(L), work.data_ptr() + GUARD, size.value,
                                      outs["total"].data_ptr() + 4 * GUARD, ctypes.byref(G), dtheta,
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
