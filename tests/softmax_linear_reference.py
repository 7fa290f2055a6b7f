"""
References for mi_softmax_linear_forward (Categorical(logits = X @ Theta), Theta [K, P, C]):

* ``reference``: fp64, with the two error scales of the GPU test,
      tbound[k]       = |site_scale| * sum_i mask_i (|eta_y| + |m| + |log s|)
      bound[k, p, c]  = |site_scale| * sum_i mask_i |d_c| |X_ip| + 1e-6
  (m = max_c eta_c, s = sum_c exp(eta_c - m), d_c = [c == y_i] - exp(eta_c - m) / s);
* ``float32_restatement``: the kernel's formula in float32 -- eta as the fmaf chain over the
  features in order (what v_mfma_f32_32x32x2_f32 computes), the elementwise step (max, exp, sum,
  log, quotient) in float32, the sums over rows in fp64;
* ``launch``: one launch through the C ABI over poisoned buffers: NaN-filled outputs and guard
  bytes on both sides of the workspace.

Labels outside [0, C) (only ever met on masked-out rows here, or in the flag tests, which do not
compare values) count as no category.
"""
import ctypes
from collections import namedtuple

import numpy as np

from mininf_amd import _native as nat

GUARD = 256
Result = namedtuple("Result", "rc total dtheta flags")


def _gather(X, y, mask, row_index):
    if mask is None:
        mask = np.ones(X.shape[0], bool)
    if row_index is not None:
        X, y, mask = X[row_index], y[row_index], mask[row_index]
    return X, y, mask.astype(bool)


def _labels(y, mask, C):
    """int labels, -1 where masked out or outside [0, C)."""
    with np.errstate(invalid="ignore"):
        yi = np.where(mask & (y >= 0) & (y < C) & (y == np.floor(y)), y, -1)
    return np.nan_to_num(yi, nan=-1.0).astype(np.int64)


def reference(X, theta, y, mask, site_scale, g0, row_index=None):
    """(total [K], dtheta [K, P, C], tbound [K], bound [K, P, C]) in fp64."""
    X, y, m = _gather(X, y, mask, row_index)
    X = X.astype(np.float64)
    theta = theta.astype(np.float64)
    C = theta.shape[2]
    lab = _labels(y, m, C)
    eta = np.einsum("ip,kpc->kic", X, theta)
    mx = eta.max(-1, keepdims=True)
    e = np.exp(eta - mx)
    s = e.sum(-1, keepdims=True)
    onehot = (lab[:, None] == np.arange(C)[None, :]).astype(np.float64)   # [N, C]
    eta_y = (eta * onehot[None]).sum(-1)
    obs = m.astype(np.float64)[None, :]
    lp = (eta_y - mx[..., 0] - np.log(s[..., 0])) * obs
    d = (onehot[None] - e / s) * obs[..., None]                           # [K, N, C]
    total = site_scale * lp.sum(1)
    dtheta = g0 * site_scale * np.einsum("kic,ip->kpc", d, X)
    tbound = abs(site_scale) * ((np.abs(eta_y) + np.abs(mx[..., 0]) + np.abs(np.log(s[..., 0]))) * obs).sum(1)
    bound = abs(site_scale) * np.einsum("kic,ip->kpc", np.abs(d), np.abs(X)) + 1e-6
    return total, dtheta, tbound, bound


def float32_restatement(X, theta, y, mask, site_scale, g0, row_index=None):
    """(total [K], dtheta [K, P, C]) by the kernel's float32 formula."""
    f = np.float32
    X, y, m = _gather(X, y, mask, row_index)
    X = X.astype(f)
    theta = theta.astype(f)
    K, P, C = theta.shape
    lab = _labels(y, m, C)
    eta = np.zeros((K, X.shape[0], C), f)
    for j in range(P):   # one rounding per step: the product is exact in fp64
        eta = (eta.astype(np.float64) +
               X[None, :, j, None].astype(np.float64) * theta[:, None, j, :].astype(np.float64)).astype(f)
    mx = eta.max(-1, keepdims=True)
    e = np.exp((eta - mx).astype(f)).astype(f)
    s = np.zeros(mx.shape, f)
    for c in range(C):   # the running sum over the categories in order
        s = (s + e[..., c:c + 1]).astype(f)
    ls = np.log(s).astype(f)
    pc = (e * (f(1) / s).astype(f)).astype(f)
    onehot = (lab[:, None] == np.arange(C)[None, :])
    d = np.where(m[None, :, None], (onehot[None].astype(f) - pc).astype(f), f(0))
    eta_y = (eta.astype(np.float64) * onehot[None]).sum(-1)
    lp = np.where(m[None, :], eta_y - mx[..., 0].astype(np.float64) - ls[..., 0].astype(np.float64), 0.0)
    total = site_scale * lp.sum(1)
    dtheta = g0 * site_scale * np.einsum("kic,ip->kpc", d.astype(np.float64), X.astype(np.float64))
    return total, dtheta


def describe(X, theta, y, mask, site_scale, g0, row_index=None):
    """The mi_softmax_linear of device (or host: invalid-argument tests) tensors."""
    import torch
    L = nat.SoftmaxLinear()
    L.K, L.P, L.C = theta.shape
    L.N = X.shape[0] if row_index is None else row_index.shape[0]
    L.x = X.data_ptr()
    L.x_stride_i, L.x_stride_j = X.stride()
    L.theta = theta.data_ptr()
    L.theta_stride_k, L.theta_stride_j, L.theta_stride_c = theta.stride()
    L.value = y.data_ptr()
    L.value_stride_i = y.stride(0)
    assert y.dtype in (torch.int64, torch.float32)
    L.value_kind = nat.SOFTMAX_LABEL_INT64 if y.dtype == torch.int64 else nat.SOFTMAX_LABEL_FLOAT32
    if mask is not None:
        assert mask.dtype in (torch.uint8, torch.bool)
        L.mask = mask.data_ptr()
        L.mask_stride_i = mask.stride(0)
    if row_index is not None:
        assert row_index.dtype == torch.int32 and row_index.is_contiguous()
        L.row_index = row_index.data_ptr()
    L.grad_scale = g0
    L.site_scale = site_scale
    return L


def launch(X, theta, y, mask, site_scale, g0, row_index=None, grads=True):
    """One mi_softmax_linear_forward over poisoned buffers."""
    import torch
    device = X.device
    L = describe(X, theta, y, mask, site_scale, g0, row_index)
    K, P, C = theta.shape
    lib = nat.lib()
    size = ctypes.c_size_t()
    nat.check(lib.mi_softmax_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "workspace")
    work = torch.full((size.value + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert (work.data_ptr() + GUARD) % 256 == 0
    total = torch.full((K,), float("nan"), device=device)
    dtheta = torch.full((K, P, C), float("nan"), device=device)
    flags = torch.full((1,), -1, dtype=torch.int32, device=device)
    rc = lib.mi_softmax_linear_forward(ctypes.byref(L), work.data_ptr() + GUARD, size.value,
                                       total.data_ptr(), dtheta.data_ptr() if grads else None,
                                       flags.data_ptr(), nat.stream_handle(device))
    torch.cuda.synchronize()
    assert bool((work[:GUARD] == 0xFF).all()), "the launch wrote below its workspace"
    assert bool((work[GUARD + size.value:] == 0xFF).all()), "the launch wrote past its workspace"
    if not grads or rc != 0:
        assert bool(torch.isnan(dtheta).all()), "dtheta written although it was not passed"
    return Result(rc, total.cpu().numpy(), dtheta.cpu().numpy(), int(flags.cpu()[0]) & 0xFFFFFFFF)
