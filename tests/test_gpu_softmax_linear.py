"""
mi_softmax_linear_forward (csrc/softmax_linear.hip: Categorical(logits = X @ Theta) on the matrix
cores) point by point against the fp64 reference of tests/softmax_linear_reference.py, through the
C ABI and over poisoned buffers.

Shapes: an orthogonal thinning of N x K x P x C over the smallest sizes that can break the tiling
(every pair of values of two dimensions occurs), N = 700 giving three row stages of 256 rows (six
of 128 with two feature tiles), plus one launch whose row blocks run two stages each (the partial
tile accumulated across stages). Operands, regimes and flags as listed in CASES below.

Bounds (the project's own, tests/test_gpu_count_linear.py): |total - ref| <= 1e-5 * tbound and
|dtheta - ref| <= 1e-5 * |g0| * bound + 1e-7, with tbound and bound from the reference. Every launch
is also compared, within the same bounds, with mi_categorical_forward run on the materialised
float32 logits (its dlogits contracted with X in fp64). test_softmax_linear_host.py holds a float32
restatement of the kernel's formula to both bounds on these inputs without a GPU.

The regimes with large logits (spread, offset) use dyadic X and Theta, so that every eta is exact in
float32: a float32 eta of magnitude 1e4 otherwise carries an error of 1e-3, which no float32
kernel can keep out of the softmax.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests.softmax_linear_reference import launch, reference

SITE_SCALE = 3.0
G0 = -0.25
TOL = 1e-5


@dataclasses.dataclass(frozen=True)
class Case:
    N: int
    K: int
    P: int
    C: int
    regime: str = "plain"     # plain, spread, equal, offset, smallest
    xt: bool = False          # X as a transposed view of a [P, N] array
    perm: bool = False        # Theta as a permuted view of a [P, C, K] array
    floats: bool = False      # float32 labels
    mask: str = "none"        # none, random, allfalse
    rows: bool = False        # row_index: out-of-order rows with repeats into a larger dataset
    grads: bool = True        # False: dtheta NULL

    @property
    def id(self):
        parts = [f"N{self.N}_K{self.K}_P{self.P}_C{self.C}"]
        parts += [w for w, on in (("xt", self.xt), ("perm", self.perm), ("floats", self.floats),
                                  ("rows", self.rows), ("nograd", not self.grads)) if on]
        parts += [w for w in (self.regime, self.mask) if w not in ("plain", "none")]
        return "-".join(parts)


NS, KS, PS, CS = (1, 31, 33, 100, 700), (1, 5, 32, 33, 70), (1, 3, 32, 33, 64), (2, 3, 8, 9, 32)
MASKS = ("none", "random", "allfalse")


def _cases():
    out = []
    i = 0
    for a in range(5):       # strength-2 orthogonal array: columns a, b, a + b, a + 2 b (mod 5)
        for b in range(5):
            out.append(Case(NS[a], KS[b], PS[(a + b) % 5], CS[(a + 2 * b) % 5],
                            xt=i % 2 == 1, perm=(i // 2) % 2 == 1, floats=(i // 3) % 2 == 1,
                            mask=MASKS[i % 3] if i % 5 else "random", rows=i % 4 == 1,
                            grads=i % 7 != 3))
            i += 1
    for j, regime in enumerate(("spread", "equal", "offset", "smallest")):
        out += [Case(100, 5, 3, 3, regime), Case(33, 33, 33, 9, regime, floats=True, mask="random"),
                Case(700, 32, 32, 8, regime, xt=True, rows=True),
                Case(31, 70, 64, 32, regime, perm=True),
                Case(100, 1, 1, 2, regime, mask="random"),
                Case(700, 5, 64, 2 + j, regime, perm=True, xt=True)]
    out.append(Case(700, 70, 64, 32, mask="random", rows=True))
    out.append(Case(262144 + 300, 1, 3, 2, mask="random"))    # two stages per row block
    return out


CASES = _cases()
assert len(CASES) <= 100 and len({c.id for c in CASES}) == len(CASES)


def dyadic(rng, shape, scale, step=8):
    return np.round(rng.uniform(-scale, scale, shape) * step) / step


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """(X [M, P], theta [K, P, C], y [M], mask [M] or None, row_index or None), numpy; M >= N rows
    of data, of which row_index (when given) picks the launch's N."""
    rng = np.random.default_rng(CASES.index(case) + 17)
    N, K, P, C = case.N, case.K, case.P, case.C
    M = N + 37 if case.rows else N
    if case.regime in ("plain", "smallest"):
        w = 3.0 if case.regime == "smallest" else 1.0
        X = rng.standard_normal((M, P)) * 0.7
        theta = rng.standard_normal((K, P, C)) * w / np.sqrt(P)
    elif case.regime == "equal":
        X = rng.standard_normal((M, P))
        theta = np.repeat(rng.standard_normal((K, P, 1)), C, axis=2)
    else:
        X = dyadic(rng, (M, P), 2.0)
        theta = dyadic(rng, (K, P, C), 1.0)
        if case.regime == "spread":
            # feature 0 carries the spread: X in {-2, -1, 1, 2} times Theta from -40 to 40
            X[:, 0] = rng.choice([-2.0, -1.0, 1.0, 2.0], M)
            theta[:, 0, :] = np.round(40.0 * (2.0 * np.arange(C) / (C - 1) - 1.0) * 8) / 8
            theta[:, 1:, :] /= 4.0
        else:
            X[:, 0] = 1.0
            theta[:, 0, :] = 1e4
    X = X.astype(np.float32)
    theta = theta.astype(np.float32)
    y = rng.integers(0, C, M)
    row_index = None
    if case.rows:
        row_index = rng.integers(0, M, N).astype(np.int32)
        row_index[N // 2] = row_index[0]
    if case.regime == "smallest":   # the label holds particle 0's smallest logit
        y = (X.astype(np.float64) @ theta[0].astype(np.float64)).argmin(-1)
    mask = None
    if case.mask == "random":
        mask = rng.random(M) < 0.6
        y = np.where(mask, y, C + 5)        # a masked-out row's label is never looked at
    elif case.mask == "allfalse":
        mask = np.zeros(M, bool)
    y = y.astype(np.float32 if case.floats else np.int64)
    if case.floats and mask is not None:
        y[~mask] = np.nan
    return X, theta, y, mask, row_index


@functools.lru_cache(maxsize=None)
def expected(case: Case):
    X, theta, y, mask, row_index = inputs(case)
    return reference(X, theta, y.astype(np.float64), mask, SITE_SCALE, G0, row_index)


def fractions(total, dtheta, case: Case):
    """Largest |error| / bound of the total and of dtheta against the fp64 reference."""
    rt, rd, tbound, bound = expected(case)
    with np.errstate(invalid="ignore", divide="ignore"):
        ft = np.abs(total - rt) / (TOL * tbound)
        ft = np.where(np.abs(total - rt) == 0, 0.0, ft)
    fd = 0.0
    if dtheta is not None:
        fd = float((np.abs(dtheta - rd) / (TOL * abs(G0) * bound + 1e-7)).max())
    return float(np.max(ft)), fd


def on_device(case: Case, device):
    X, theta, y, mask, row_index = inputs(case)
    if case.xt:
        Xd = torch.tensor(np.ascontiguousarray(X.T), device=device).t()
    else:
        Xd = torch.tensor(X, device=device)
    if case.perm:
        td = torch.tensor(np.ascontiguousarray(theta.transpose(1, 2, 0)), device=device).permute(2, 0, 1)
    else:
        td = torch.tensor(theta, device=device)
    yd = torch.tensor(y, device=device)
    md = None if mask is None else torch.tensor(mask, device=device)
    rd = None if row_index is None else torch.tensor(row_index, device=device)
    return Xd, td, yd, md, rd


WORST = {"total": 0.0, "dtheta": 0.0, "cat_total": 0.0, "cat_dtheta": 0.0}


def categorical_on_materialised(Xd, td, yd, md, rd):
    """mi_categorical_forward on the float32 logits X @ Theta: (total, dtheta in fp64 from dlogits)."""
    if rd is not None:
        Xd, yd, md = Xd[rd.long()], yd[rd.long()], None if md is None else md[rd.long()]
    K, N, C = td.shape[0], Xd.shape[0], td.shape[2]
    logits = torch.matmul(Xd, td).contiguous()
    yi = torch.where(yd == yd, yd, torch.full_like(yd, -1)).to(torch.int64).reshape(1, N).expand(K, N)
    mk = None if md is None else md.reshape(1, N).expand(K, N)
    dlogits = torch.full_like(logits, float("nan"))
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_categorical_workspace_bytes(K, N, ctypes.byref(size)), "workspace")
    work = torch.empty(max(1, size.value), dtype=torch.uint8, device=Xd.device)
    total = torch.empty(K, device=Xd.device)
    flags = torch.empty(1, dtype=torch.int32, device=Xd.device)
    nat.check(lib.mi_categorical_forward(
        logits.data_ptr(), *logits.stride(), K, N, C, yi.data_ptr(), yi.stride(0), yi.stride(1),
        None if mk is None else mk.data_ptr(), 0 if mk is None else mk.stride(1), SITE_SCALE, G0,
        dlogits.data_ptr(), work.data_ptr(), size.value, total.data_ptr(), flags.data_ptr(),
        nat.stream_handle(Xd.device)), "mi_categorical_forward")
    dtheta = torch.einsum("kic,ip->kpc", dlogits.double(), Xd.double())
    return total.cpu().numpy(), dtheta.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_launch_matches_the_fp64_reference(case):
    device = torch.device("cuda")
    Xd, td, yd, md, rd = on_device(case, device)
    r = launch(Xd, td, yd, md, SITE_SCALE, G0, rd, grads=case.grads)
    assert r.rc == 0 and r.flags == 0
    assert np.isfinite(r.total).all()
    ft, fd = fractions(r.total.astype(np.float64),
                       r.dtheta.astype(np.float64) if case.grads else None, case)
    ct, cd = categorical_on_materialised(Xd, td, yd, md, rd)
    rt, rdt, tbound, bound = expected(case)
    gt = np.abs(r.total - ct)
    gt = float(np.max(np.where(gt == 0, 0.0, gt / np.maximum(TOL * tbound, 1e-300))))
    gd = float((np.abs(r.dtheta - cd) / (TOL * abs(G0) * bound + 1e-7)).max()) if case.grads else 0.0
    for key, value in (("total", ft), ("dtheta", fd), ("cat_total", gt), ("cat_dtheta", gd)):
        WORST[key] = max(WORST[key], value)
    print(f"\n{case.id}: fraction of the bound: total {ft:.3f} dtheta {fd:.3f}; against "
          f"mi_categorical_forward: total {gt:.3f} dtheta {gd:.3f}; worst so far {WORST}")
    assert ft <= 1.0 and fd <= 1.0, (ft, fd)
    assert gt <= 1.0 and gd <= 1.0, (gt, gd)


def _flag_launch(device, labels, observed, floats, theta_edit=None):
    """N = 40, K = 3, P = 3, C = 4 with row 7 given the label (and mask) under test."""
    rng = np.random.default_rng(5)
    X = torch.tensor(rng.standard_normal((40, 3)).astype(np.float32), device=device)
    theta = torch.tensor(rng.standard_normal((3, 3, 4)).astype(np.float32), device=device)
    if theta_edit is not None:
        theta[theta_edit] = float("inf")
    y = rng.integers(0, 4, 40).astype(np.float32 if floats else np.int64)
    y[7] = labels
    mask = np.ones(40, bool)
    mask[7] = observed
    return launch(X, theta, torch.tensor(y, device=device), torch.tensor(mask, device=device), 1.0, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("label,floats", [(-1, False), (4, False), (-1.0, True), (4.0, True),
                                          (1.5, True), (float("nan"), True)])
def test_label_outside_the_support_is_flagged_only_when_observed(label, floats):
    device = torch.device("cuda")
    r = _flag_launch(device, label, True, floats)
    assert r.rc == 0 and r.flags == nat.FLAG_SUPPORT
    r = _flag_launch(device, label, False, floats)
    assert r.rc == 0 and r.flags == 0
    assert np.isfinite(r.total).all() and np.isfinite(r.dtheta).all()


@pytest.mark.gpu
def test_infinite_theta_is_flagged():
    r = _flag_launch(torch.device("cuda"), 2, True, False, theta_edit=(1, 2, 3))
    assert r.rc == 0 and r.flags == nat.FLAG_PARAM
