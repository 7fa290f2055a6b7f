"""
mi_gather_slopes_forward (csrc/gather_linear_site.hip) point by point against the fp64 reference of
tests/gather_slopes_reference.py, through the C ABI, over poisoned and guarded buffers.

Bounds (those of tests/test_gpu_gather_site.py):
    |total - ref| <= 1e-5 * tbound,    |grad - ref| <= 1e-5 * |g0| * bound + 1e-7
with tbound / bound the reference's sums of absolute terms, dtheta's and every dslope's among them.
test_gather_slopes_host.py checks a float32 restatement of the kernel against the same bounds on
every input set below.

Shapes: a strength-2 cover of N in {1, 63, 64, 65, 257, 4 R + 3} (R = 256 sorted rows per chunk),
K in {1, 5, 33, 65}, G in {1, 2, 7, 64, 2 N} (empty groups), S in {1, 2, 3, 4} and
P in {0, 1, 8, 9, 17, 32} (the edges of the kernel's buckets); the other factors (family and role
1's kind, shift, mult, mask, the memory layouts of X, theta, the tables and the z columns, int64
values, gradients not asked for) cycle along the cases. SEGMENTS are the segment layouts of
test_gpu_gather_site.py. Every launch runs twice and is compared bit for bit.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests import gather_linear_reference as linear_ref
from tests import test_gpu_gather_site as site
from tests.gather_linear_reference import X_LAYOUTS
from tests.gather_site_reference import ROWS, sort_plan
from tests.gather_slopes_reference import (Z_LAYOUTS, _names, describe_slopes, launch, reference,
                                           slopes_tensors)
from tests.test_gpu_gather_linear_site import ROLE_SETS, add_linear

R = ROWS
NS = (1, 63, 64, 65, 257, 4 * R + 3)
KS = (1, 5, 33, 65)
SS = (1, 2, 3, 4)
PS = (0, 1, 8, 9, 17, 32)
FACTORS = (NS, KS, range(5), SS, PS)   # (the third: which of G's five values)


def add_effects(case, seed, P, x_layout="plain", theta_strided=False):
    """add_linear, or for P = 0 an empty X [N, 0] and theta [K, 0]."""
    if P > 0:
        return add_linear(case, seed, P, x_layout, theta_strided)
    case.update(P=0, X=np.zeros((case["N"], 0), np.float32), x_layout=x_layout,
                theta=np.zeros((case["K"], 0), np.float32), theta_strided=theta_strided)
    return case


# Seeds are chosen so that the float32 restatement of the kernel meets the bounds on every case
# (test_gather_slopes_host.py): case number -> what is added to its seeds.
RESEED = {16: 100, 17: 100}
ROLE_OFFSET = 1   # where the cycle of ROLE_SETS starts


def add_slopes(case, seed, S, z_layout="plain"):
    """S slope tables [K, G] and columns [N] beside a case of add_linear."""
    rng = np.random.default_rng(seed)
    case["slopes"] = [(rng.normal(0, 0.5 / np.sqrt(S), (case["K"], case["G"])).astype(np.float32),
                       rng.normal(0, 1, case["N"]).astype(np.float32)) for _ in range(S)]
    case["z_layout"] = z_layout
    return case


def _shapes():
    """(N, K, G index, S, P): every pair of values of two factors occurs. Built greedily (the
    tuple that covers the most pairs still missing, the first of them in the product's order)."""
    pairs = list(itertools.combinations(range(len(FACTORS)), 2))
    missing = {(x, y, u, v) for x, y in pairs for u in FACTORS[x] for v in FACTORS[y]}
    candidates = list(itertools.product(*FACTORS))
    out = []
    while missing:
        best = max(candidates, key=lambda t: sum((x, y, t[x], t[y]) in missing for x, y in pairs))
        out.append(best)
        missing -= {(x, y, best[x], best[y]) for x, y in pairs}
    for x, y in pairs:
        have = {(s[x], s[y]) for s in out}
        assert len(have) == len(FACTORS[x]) * len(FACTORS[y]), (x, y)
    return out


def _cases():
    out = {}
    for n, (N, K, b, S, P) in enumerate(_shapes()):
        G = (1, 2, 7, 64, 2 * N)[b]
        family, *kinds = ROLE_SETS[(n + ROLE_OFFSET) % len(ROLE_SETS)]
        pattern = site.PATTERNS[(n // 2) % len(site.PATTERNS)]
        rng = np.random.default_rng(4000 + n)
        seed = n + RESEED.get(n, 0)
        case = site.make_case(seed, family, [k for k in kinds if k], K, N, G,
                              site.make_index(rng, pattern, N, G), shift=site.TERMS[n % 3],
                              mult=site.TERMS[(n // 3) % 3],
                              mask=("none", "random", "none", "false")[n % 4],
                              strided=n % 5 == 1, int_values=n % 2 == 0,
                              site_scale=(1.0, 2.5)[n % 2])
        add_effects(case, 5000 + seed, P, X_LAYOUTS[n % len(X_LAYOUTS)], theta_strided=n % 4 == 1)
        # the columns of one [N, S] matrix in every other case, one case a float off alignment
        add_slopes(case, 6000 + seed, S, "offset" if n == 4 else Z_LAYOUTS[n % 2])
        if n % 7 == 3:   # some gradients not asked for
            case["null"] = tuple(list(_names(case))[::2])
        elif n % 7 == 5:
            case["null"] = ("dtheta", f"slope{S - 1}")
        elif n % 7 == 6:
            case["null_slopes"] = True
        out[f"{family}-{''.join(k or '' for k in kinds)}-N{N}-K{K}-G{G}-S{S}-P{P}-{pattern}-"
            f"{case['z_layout']}-{n}"] = case
    return out


def _segment_cases():
    out = {}
    sets = {"normal": ROLE_SETS[0], "bernoulli": ROLE_SETS[2], "poisson": ROLE_SETS[4]}
    for j, (name, base) in enumerate(site._segment_cases().items()):
        family, *kinds = sets[base["family"]] if j != 1 else ROLE_SETS[5]
        case = site.make_case(700 + j, family, [k for k in kinds if k], base["K"], base["N"],
                              base["G"], base["index"], shift=site.TERMS[j % 3],
                              mult=site.TERMS[(j + 1) % 3], mask=("none", "random")[j % 2],
                              int_values=True)
        add_effects(case, 800 + j, (0, 8, 17, 1, 9)[j], X_LAYOUTS[j % len(X_LAYOUTS)])
        out[f"slopes-{name}"] = add_slopes(case, 900 + j, (1, 2, 4, 3, 2)[j],
                                           Z_LAYOUTS[j % len(Z_LAYOUTS)])
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


def wanted(case):
    return {"total", *(n for n in _names(case) if n not in case["null"] and
                       not (n.startswith("slope") and case.get("null_slopes")))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gather_slopes_against_reference(name):
    case = CASES[name]
    device = torch.device("cuda")
    rc, got, flags = launch(case, device)
    assert rc == 0 and flags == 0, (rc, flags)
    assert set(got) == wanted(case)
    print(name, check(case, got))
    # a group without rows is exactly 0, in every table
    present = np.zeros(case["G"], bool)
    present[np.where(case["index"] < 0, case["index"] + case["G"], case["index"])] = True
    if case["mask"] is not None and not case["mask"].any():
        present[:] = False   # (an all-false mask gives zeros)
        if "dtheta" in got:
            assert np.all(got["dtheta"] == 0.0)
    for key, value in got.items():
        if value.ndim == 2 and key != "dtheta":
            assert np.all(value[:, ~present] == 0.0), key
    rc2, again, _ = launch(case, device)
    assert rc2 == 0
    for key in got:   # bit for bit
        assert np.array_equal(got[key].view(np.uint32), again[key].view(np.uint32)), key


def small_case(family="normal", S=2, P=3, seed=40):
    """N = 257 (two chunks), K = 5, G = 7."""
    N, K, G = 257, 5, 7
    rng = np.random.default_rng(seed)
    kinds = {"normal": ["g", "p"], "bernoulli": ["g"], "poisson": ["g"]}[family]
    case = site.make_case(seed, family, kinds, K, N, G, site.make_index(rng, "random", N, G),
                          shift="pointer", mult="pointer")
    return add_slopes(add_effects(case, seed + 1, P), seed + 2, S)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
def test_zero_columns_reproduce_the_linear_site(family):
    """With every z_s identically 0 (fmaf(b, 0, eta) == eta) the shared path gives
    mi_gather_linear_forward's words, and every dslope is exactly 0."""
    device = torch.device("cuda")
    case = small_case(family, S=4, P=3)
    case["slopes"] = [(beta, np.zeros_like(z)) for beta, z in case["slopes"]]
    rc, got, flags = launch(case, device)
    assert rc == 0 and flags == 0, (rc, flags)
    rc, want, flags = linear_ref.launch(case, device)
    assert rc == 0 and flags == 0, (rc, flags)
    for key, value in want.items():
        assert np.array_equal(got[key].view(np.uint32), value.view(np.uint32)), key
    for s in range(4):
        assert np.all(got[f"slope{s}"] == 0.0), s


def slopes_site(device="cpu", **changes):
    """A valid mi_gather_slopes over tensors on ``device`` with ``changes`` applied: "S" of the
    struct itself, "slope0.z" of a slope, "linear.P" of its mi_gather_linear, "site.N" of its
    mi_gather_site, "role0.kind" of a role."""
    case = small_case()
    tensors = slopes_tensors(case, device)
    order, sg = (torch.from_numpy(x).to(device) for x in sort_plan(case["index"], case["G"]))
    M = describe_slopes(case, tensors, order, sg)
    for name, value in changes.items():
        target = M
        *path, leaf = name.split(".")
        for part in path:
            target = M.linear if part == "linear" else M.linear.site if part == "site" else \
                M.slope[int(part[-1])] if part.startswith("slope") else \
                M.linear.site.role[int(part[-1])]
        setattr(target, leaf, value)
    return M, (tensors, order, sg)


INVALID = [
    {"site.K": 0}, {"site.N": 0}, {"site.G": 0}, {"site.family": 3}, {"site.order": None},
    {"site.sorted_group": None}, {"site.value": None}, {"site.value_kind": 2},
    {"role0.kind": 4}, {"role0.data": None}, {"role1.data": None}, {"role0.link": 2},
    {"role0.shift_kind": 3}, {"role0.mult_kind": -1}, {"role0.shift": None}, {"role0.mult": None},
    # mi_gather_slopes' own: role 0 is not a GATHER role, S < 1, a NULL table or z among the first
    # S, P < 0, P >= 1 without X or theta
    {"role0.kind": nat.GATHER_PARTICLE}, {"role0.kind": nat.GATHER_DATA},
    {"role0.kind": nat.GATHER_CONSTANT}, {"S": 0}, {"S": -1}, {"slope0.table": None},
    {"slope1.z": None}, {"S": 3}, {"linear.P": -1}, {"linear.x": None}, {"linear.theta": None}]


def argument_errors(device):
    """Every invalid-argument return of the two entry points, over buffers that must stay as they
    are: nothing is launched."""
    lib = nat.lib()
    size = ctypes.c_size_t()
    work = torch.full((1 << 17,), 0x5A, dtype=torch.uint8, device=device)
    total = torch.full((5,), 7.0, device=device)
    dtheta = torch.full((5, 33), 7.0, device=device)
    tables = torch.full((4, 5, 7), 7.0, device=device)
    dslope = (nat.c_vp * nat.GATHER_MAX_SLOPES)(*(tables[s].data_ptr() for s in range(4)))
    flags = torch.full((1,), 9, dtype=torch.int32, device=device)
    fwd = lib.mi_gather_slopes_forward

    def forward(M, workspace=work.data_ptr(), bytes_=work.numel(), total_=total.data_ptr(),
                flags_=flags.data_ptr()):
        return fwd(ctypes.byref(M) if M is not None else None, workspace, bytes_, total_, None,
                   dtheta.data_ptr(), dslope, flags_,
                   nat.stream_handle(device) if device != "cpu" else None)
    for changes in INVALID:
        M, keep = slopes_site(device, **changes)
        assert lib.mi_gather_slopes_workspace_bytes(ctypes.byref(M), ctypes.byref(size)) == \
            nat.MI_EINVAL, changes
        assert forward(M) == nat.MI_EINVAL, changes
    M, keep = slopes_site(device)
    assert lib.mi_gather_slopes_workspace_bytes(ctypes.byref(M), None) == nat.MI_EINVAL
    assert lib.mi_gather_slopes_workspace_bytes(None, ctypes.byref(size)) == nat.MI_EINVAL
    assert forward(None) == nat.MI_EINVAL
    assert forward(M, total_=None) == nat.MI_EINVAL
    assert forward(M, flags_=None) == nat.MI_EINVAL
    assert lib.mi_gather_slopes_workspace_bytes(ctypes.byref(M), ctypes.byref(size)) == 0
    assert 0 < size.value <= work.numel()
    assert forward(M, workspace=None) == nat.MI_EWORKSPACE
    assert forward(M, bytes_=size.value - 1) == nat.MI_EWORKSPACE
    for changes in ({"linear.P": nat.GATHER_LINEAR_MAX_P + 1}, {"S": nat.GATHER_MAX_SLOPES + 1}):
        big, keep2 = slopes_site(device, **changes)
        if "S" in changes:   # (its first four slopes are valid)
            for s in (2, 3):
                big.slope[s] = big.slope[0]
        assert lib.mi_gather_slopes_workspace_bytes(ctypes.byref(big), ctypes.byref(size)) == \
            nat.MI_EUNSUPPORTED, changes
        assert forward(big) == nat.MI_EUNSUPPORTED, changes
    if device != "cpu":
        torch.cuda.synchronize()
    assert bool((work == 0x5A).all()) and bool((total == 7.0).all()) and \
        bool((dtheta == 7.0).all()) and bool((tables == 7.0).all()) and int(flags.cpu()[0]) == 9


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    argument_errors(torch.device("cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_slope_entry_flags_observed_rows_only(family, bad):
    """A non-finite beta_s entry of a populated group sets MI_FLAG_PARAM; the same entry in a group
    whose rows are all masked out sets nothing, and a non-finite z on a masked-out row neither."""
    device = torch.device("cuda")
    case = small_case(family, S=2, P=0)
    group = 3
    rows = np.where(case["index"] < 0, case["index"] + case["G"], case["index"]) == group
    assert rows.any()
    case["slopes"][1][0][2, group] = bad
    rc, _, flags = launch(case, device)
    assert rc == 0 and flags == nat.FLAG_PARAM, (rc, flags)
    case["mask"] = ~rows
    case["slopes"][0][1][rows] = bad   # (z on masked-out rows: never read)
    rc, got, flags = launch(case, device)
    assert rc == 0 and flags == 0, (rc, flags)
    assert all(np.isfinite(value).all() for value in got.values())
    assert all(np.all(got[f"slope{s}"][:, group] == 0.0) for s in range(2))
