"""
mi_gather_linear_forward (csrc/gather_linear_site.hip) point by point against the fp64 reference of
tests/gather_linear_reference.py, through the C ABI, over poisoned and guarded buffers.

Bounds (those of tests/test_gpu_gather_site.py):
    |total - ref| <= 1e-5 * tbound,    |grad - ref| <= 1e-5 * |g0| * bound + 1e-7
with tbound / bound the reference's sums of absolute terms, dtheta's among them.
test_gather_linear_host.py checks a float32 restatement of the kernel against the same bounds on
every input set below.

Shapes: a strength-2 cover of N in {1, 63, 64, 65, 257, 4 R + 3} (R = 256 sorted rows per chunk),
K in {1, 5, 33, 65}, G in {1, 2, 7, 64, 2 N} (empty groups) and P in {1, 3, 8, 9, 16, 17, 32} (the
edges of the kernel's P buckets); the other factors (family and role 1's kind, shift, mult, mask,
the memory layouts of X, theta and the tables, int64 values, gradients not asked for) cycle along
the cases. SEGMENTS are the segment layouts of test_gpu_gather_site.py. Every launch runs twice and
is compared bit for bit.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests import test_gpu_gather_site as site
from tests.gather_linear_reference import (X_LAYOUTS, _names, describe_linear, launch,
                                           linear_tensors, reference)
from tests.gather_site_reference import ROWS, sort_plan

R = ROWS
NS = (1, 63, 64, 65, 257, 4 * R + 3)
KS = (1, 5, 33, 65)
PS = (1, 3, 8, 9, 16, 17, 32)
# (family, role 0, role 1): role 0 is the gathered predictor with the linear term
ROLE_SETS = (("normal", "g", "p"), ("normal", "g", "c"), ("bernoulli", "g", None),
             ("normal", "g", "d"), ("poisson", "g", None), ("normal", "g", "g"))


def add_linear(case, seed, P, x_layout="plain", theta_strided=False):
    """X [N, P] and theta [K, P] beside a case of test_gpu_gather_site.make_case."""
    rng = np.random.default_rng(seed)
    case["P"] = P
    case["X"] = rng.normal(0, 1, (case["N"], P)).astype(np.float32)
    case["theta"] = rng.normal(0, 0.5 / np.sqrt(P), (case["K"], P)).astype(np.float32)
    case["x_layout"] = x_layout
    case["theta_strided"] = theta_strided
    return case


def _shapes():
    """(N, K, G index, P): every pair of values of two factors occurs."""
    out = [(NS[a], KS[(a + 3 * p) % 4], (a + p) % 5, PS[p]) for a in range(6) for p in range(7)]
    for x, y in itertools.combinations(range(4), 2):
        have = {(s[x], s[y]) for s in out}
        sizes = [len(v) for v in (NS, KS, range(5), PS)]
        assert len(have) == sizes[x] * sizes[y], (x, y)
    return out


def _cases():
    out = {}
    for n, (N, K, b, P) in enumerate(_shapes()):
        G = (1, 2, 7, 64, 2 * N)[b]
        family, *kinds = ROLE_SETS[n % len(ROLE_SETS)]
        pattern = site.PATTERNS[(n // 2) % len(site.PATTERNS)]
        rng = np.random.default_rng(2000 + n)
        case = site.make_case(n, family, [k for k in kinds if k], K, N, G,
                              site.make_index(rng, pattern, N, G), shift=site.TERMS[n % 3],
                              mult=site.TERMS[(n // 3) % 3],
                              mask=("none", "random", "none", "false")[n % 4],
                              strided=n % 5 == 1, int_values=n % 2 == 0,
                              site_scale=(1.0, 2.5)[n % 2])
        add_linear(case, 3000 + n, P, X_LAYOUTS[n % len(X_LAYOUTS)], theta_strided=n % 4 == 1)
        if n % 7 == 3:   # some gradients not asked for
            case["null"] = tuple(list(_names(case))[::2])
        elif n % 7 == 5:
            case["null"] = ("dtheta",)
        out[f"{family}-{''.join(k or '' for k in kinds)}-N{N}-K{K}-G{G}-P{P}-{pattern}-"
            f"{case['x_layout']}-{n}"] = case
    return out


def _segment_cases():
    out = {}
    sets = {"normal": ROLE_SETS[0], "bernoulli": ROLE_SETS[2], "poisson": ROLE_SETS[4]}
    for j, (name, base) in enumerate(site._segment_cases().items()):
        family, *kinds = sets[base["family"]] if j != 1 else ROLE_SETS[5]
        case = site.make_case(500 + j, family, [k for k in kinds if k], base["K"], base["N"],
                              base["G"], base["index"], shift=site.TERMS[j % 3],
                              mult=site.TERMS[(j + 1) % 3], mask=("none", "random")[j % 2],
                              int_values=True)
        out[f"linear-{name}"] = add_linear(case, 600 + j, (3, 8, 17, 32, 9)[j],
                                           X_LAYOUTS[j % len(X_LAYOUTS)])
    return out


CASES = {**_cases(), **_segment_cases()}


def check(case, got, what="kernel"):
    """Every output of a launch (or of the restatement) against the reference's bounds."""
    ref = reference(case)
    g0 = abs(case["g0"])
    worst = {}
    for name, value in got.items():
        want, bound = ref[name]
        if name == "total":
            err, tol = np.abs(value - want), 1e-5 * bound
        else:
            err, tol = np.abs(value - want), 1e-5 * g0 * bound + 1e-7
        worst[name] = float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0
        assert np.all(err <= tol), f"{what} {name}: {worst[name]:.3g} of its bound"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gather_linear_against_reference(name):
    case = CASES[name]
    device = torch.device("cuda")
    rc, got, flags = launch(case, device)
    assert rc == 0 and flags == 0, (rc, flags)
    assert set(got) == {"total", *(n for n in _names(case) if n not in case["null"])}
    print(name, check(case, got))
    # a group without rows is exactly 0
    present = np.zeros(case["G"], bool)
    present[np.where(case["index"] < 0, case["index"] + case["G"], case["index"])] = True
    if case["mask"] is not None and not case["mask"].any():
        present[:] = False
        if "dtheta" in got:
            assert np.all(got["dtheta"] == 0.0)
    for key, value in got.items():
        if value.ndim == 2 and key != "dtheta":
            assert np.all(value[:, ~present] == 0.0), key
    rc2, again, _ = launch(case, device)
    assert rc2 == 0
    for key in got:   # bit for bit
        assert np.array_equal(got[key].view(np.uint32), again[key].view(np.uint32)), key


def _flag_case(family, bad, masked):
    N, K, G, P = 70, 5, 3, 9
    rng = np.random.default_rng(7)
    kinds = {"normal": ["g", "p"], "bernoulli": ["g"], "poisson": ["g"]}[family]
    case = site.make_case(300, family, kinds, K, N, G, site.make_index(rng, "random", N, G))
    add_linear(case, 301, P)
    row = 37
    mask = np.ones(N, bool)
    if bad == "support":
        case["value"][row] = {"normal": np.nan, "bernoulli": 0.5, "poisson": 1.5}[family]
    elif bad == "theta":   # every row of that particle has a non-finite eta
        case["theta"][2, 4] = np.inf
        mask[:] = not masked
    else:
        case["X"][row, P - 1] = np.nan if bad == "x_nan" else -np.inf
    if masked:
        mask[row] = False
    case["mask"] = mask
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
@pytest.mark.parametrize("bad, bit", [("support", nat.FLAG_SUPPORT), ("theta", nat.FLAG_PARAM),
                                      ("x_nan", nat.FLAG_PARAM), ("x_inf", nat.FLAG_PARAM)])
def test_flags_on_observed_rows_only(family, bad, bit):
    device = torch.device("cuda")
    rc, _, flags = launch(_flag_case(family, bad, False), device)
    assert rc == 0 and flags == bit, (rc, flags)
    rc, got, flags = launch(_flag_case(family, bad, True), device)
    assert rc == 0 and flags == 0, (rc, flags)
    assert all(np.isfinite(value).all() for value in got.values())


def linear_site(device="cpu", **changes):
    """A valid mi_gather_linear over tensors on ``device`` with ``changes`` applied: "P", "x", ...
    of the struct itself, "site.N" of its mi_gather_site, "role0.kind" of a role."""
    case = site.make_case(0, "normal", ["g", "p"], 3, 10, 4, np.arange(10) % 4, shift="pointer",
                          mult="pointer")
    add_linear(case, 1, 5)
    tensors = linear_tensors(case, device)
    order, sg = (torch.from_numpy(x).to(device) for x in sort_plan(case["index"], 4))
    L = describe_linear(case, tensors, order, sg)
    for name, value in changes.items():
        target = L
        *path, leaf = name.split(".")
        for part in path:
            target = target.site if part == "site" else target.site.role[int(part[-1])]
        setattr(target, leaf, value)
    return L, (tensors, order, sg)


INVALID = [
    {"site.K": 0}, {"site.N": 0}, {"site.G": 0}, {"site.family": 3}, {"site.order": None},
    {"site.sorted_group": None}, {"site.value": None}, {"site.value_kind": 2},
    {"role0.kind": 4}, {"role0.data": None}, {"role1.data": None}, {"role0.link": 2},
    {"role0.shift_kind": 3}, {"role0.mult_kind": -1}, {"role0.shift": None}, {"role0.mult": None},
    # mi_gather_linear's own: role 0 is not a GATHER role, P < 1, no X, no theta
    {"role0.kind": nat.GATHER_PARTICLE}, {"role0.kind": nat.GATHER_DATA},
    {"role0.kind": nat.GATHER_CONSTANT}, {"P": 0}, {"P": -1}, {"x": None}, {"theta": None}]


def argument_errors(device):
    """Every invalid-argument return of the two entry points, over buffers that must stay as they
    are: nothing is launched."""
    lib = nat.lib()
    size = ctypes.c_size_t()
    work = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=device)
    total = torch.full((3,), 7.0, device=device)
    dtheta = torch.full((3, 33), 7.0, device=device)
    flags = torch.full((1,), 9, dtype=torch.int32, device=device)
    fwd = lib.mi_gather_linear_forward

    def forward(L, workspace=work.data_ptr(), bytes_=work.numel(), total_=total.data_ptr(),
                flags_=flags.data_ptr()):
        return fwd(ctypes.byref(L) if L is not None else None, workspace, bytes_, total_, None,
                   dtheta.data_ptr(), flags_, nat.stream_handle(device) if device != "cpu" else None)
    for changes in INVALID:
        L, keep = linear_site(device, **changes)
        assert lib.mi_gather_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == \
            nat.MI_EINVAL, changes
        assert forward(L) == nat.MI_EINVAL, changes
    L, keep = linear_site(device)
    assert lib.mi_gather_linear_workspace_bytes(ctypes.byref(L), None) == nat.MI_EINVAL
    assert lib.mi_gather_linear_workspace_bytes(None, ctypes.byref(size)) == nat.MI_EINVAL
    assert forward(None) == nat.MI_EINVAL
    assert forward(L, total_=None) == nat.MI_EINVAL
    assert forward(L, flags_=None) == nat.MI_EINVAL
    assert lib.mi_gather_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == 0
    assert 0 < size.value <= work.numel()
    assert forward(L, workspace=None) == nat.MI_EWORKSPACE
    assert forward(L, bytes_=size.value - 1) == nat.MI_EWORKSPACE
    big, keep2 = linear_site(device, P=nat.GATHER_LINEAR_MAX_P + 1)
    assert lib.mi_gather_linear_workspace_bytes(ctypes.byref(big), ctypes.byref(size)) == \
        nat.MI_EUNSUPPORTED
    assert forward(big) == nat.MI_EUNSUPPORTED
    if device != "cpu":
        torch.cuda.synchronize()
    assert bool((work == 0x5A).all()) and bool((total == 7.0).all()) and \
        bool((dtheta == 7.0).all()) and int(flags.cpu()[0]) == 9


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    argument_errors(torch.device("cuda"))
