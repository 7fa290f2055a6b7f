"""
mi_gather_site_forward (csrc/gather_site.hip) point by point against the fp64 reference of
tests/gather_site_reference.py, through the C ABI, over poisoned and guarded buffers.

Bounds (those of tests/test_gpu_count_linear.py):
    |total - ref| <= 1e-5 * tbound,    |grad - ref| <= 1e-5 * |g0| * bound + 1e-7
with tbound / bound the reference's sums of absolute terms. test_gather_site_host.py checks a
float32 restatement of the kernel against the same bounds on every input set below.

Shapes: a strength-2 cover of N in {1, 63, 64, 65, 257, 4 R + 3} (R = 256 sorted rows per chunk),
K in {1, 5, 33, 65} (33 and 65: just past a half and a whole 64-particle tile) and G in
{1, 2, 7, 64, 2 N} (empty groups); the other factors cycle along the cases. SEGMENTS places groups
of 63 .. 257 rows on and off the wave and chunk edges and one over rows R - 1 .. 3 R + 1.
Every launch runs twice and is compared bit for bit.
"""
import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests.gather_site_reference import ROWS, _names, launch, reference

R = ROWS
NS = (1, 63, 64, 65, 257, 4 * R + 3)
KS = (1, 5, 33, 65)
PATTERNS = ("one", "each", "sorted", "reversed", "random", "negative")
# (family, role 0, role 1): g = gathered, p = per particle, d = data, c = constant
ROLE_SETS = (("normal", "g", "p"), ("normal", "g", "c"), ("normal", "g", "d"), ("normal", "p", "g"),
             ("normal", "d", "g"), ("normal", "c", "g"), ("normal", "g", "g"),
             ("bernoulli", "g", None), ("poisson", "g", None))
TERMS = ("none", "pointer", "constant")


def make_index(rng, pattern, N, G):
    if pattern == "one":
        return np.full(N, G - 1, np.int64)
    if pattern == "each":
        return (np.arange(N) % G).astype(np.int64)
    if pattern == "sorted":
        return np.sort(rng.integers(0, G, N)).astype(np.int64)
    if pattern == "reversed":
        return np.sort(rng.integers(0, G, N))[::-1].astype(np.int64).copy()
    index = rng.integers(0, G, N).astype(np.int64)
    if pattern == "negative":
        index = np.where(rng.random(N) < 0.5, index - G, index)
    return index


def make_case(seed, family, kinds, K, N, G, index, shift="none", mult="none", mask="none",
              strided=False, int_values=False, null=(), site_scale=1.0):
    rng = np.random.default_rng(seed)

    def term(kind, lo, hi):
        if kind == "pointer":
            return rng.uniform(lo, hi, K).astype(np.float32)
        return None if kind == "none" else float(np.float32(rng.uniform(lo, hi)))

    roles = []
    for r, kind in enumerate(kinds):
        positive = family == "normal" and r == 1
        if kind == "g":
            table = rng.normal(0, 0.7, (K, G)).astype(np.float32)
            # a gathered scale goes through exp; a Poisson rate always does
            link = "exp" if positive or family == "poisson" else "identity"
            roles.append(("gather", table, term(shift, -0.5, 0.5), term(mult, 0.5, 1.5), link))
        elif kind == "p":
            q = rng.uniform(0.5, 2.0, K) if positive else rng.normal(0, 1, K)
            roles.append(("particle", q.astype(np.float32)))
        elif kind == "d":
            q = rng.uniform(0.5, 2.0, N) if positive else rng.normal(0, 1, N)
            roles.append(("data", q.astype(np.float32)))
        else:
            roles.append(("constant", 1.3 if positive else 0.0))
    if family == "normal":
        value = rng.normal(0, 1.5, N).astype(np.float32)
    elif family == "bernoulli":
        value = (rng.random(N) < 0.4).astype(np.float32)
    else:
        value = rng.poisson(2.0, N).astype(np.int64 if int_values else np.float32)
    m = None if mask == "none" else (rng.random(N) < 0.7) if mask == "random" else np.zeros(N, bool)
    return dict(family=family, K=K, N=N, G=G, index=index, roles=roles, value=value, mask=m,
                site_scale=site_scale, g0=-1.0 / K, strided=strided, null=tuple(null))


def _cases():
    out = {}
    n = 0
    for a, N in enumerate(NS):
        for b in range(5):
            G = (1, 2, 7, 64, 2 * N)[b]
            K = KS[(a + b) % 4]
            family, *kinds = ROLE_SETS[n % len(ROLE_SETS)]
            pattern = PATTERNS[(n // 2) % len(PATTERNS)]
            rng = np.random.default_rng(1000 + n)
            case = make_case(n, family, [k for k in kinds if k], K, N, G,
                             make_index(rng, pattern, N, G), shift=TERMS[n % 3],
                             mult=TERMS[(n // 3) % 3], mask=("none", "random", "none", "false")[n % 4],
                             strided=n % 5 == 1, int_values=n % 2 == 0,
                             site_scale=(1.0, 2.5)[n % 2])
            if n % 7 == 3:   # some gradients not asked for
                case["null"] = tuple(list(_names(case))[::2])
            out[f"{family}-{''.join(k or '' for k in kinds)}-N{N}-K{K}-G{G}-{pattern}-{n}"] = case
            n += 1
    return out


def _segment_cases():
    """Groups of exactly 64, 128 and R rows and of those lengths +- 1, starting on and off the wave
    and chunk edges, and one group over rows R - 1 .. 3 R + 1 of the sorted order."""
    out = {}
    N = 4 * R + 3
    layouts = {
        "exact": [64, 128, R, 64, 128, R],
        "minus": [63, 127, R - 1, 1, 64, 128, R],
        "plus": [65, 129, R + 1, 63, 128, R],
        "offset": [3, 64, 128, R, 61, R],
        "span": [R - 1, 2 * R + 3],
    }
    for j, (name, lengths) in enumerate(layouts.items()):
        lengths = list(lengths) + [N - sum(lengths)]
        assert lengths[-1] > 0
        sorted_index = np.repeat(np.arange(len(lengths)) * 2, lengths)   # odd groups stay empty
        rng = np.random.default_rng(50 + j)
        index = sorted_index[rng.permutation(N)]
        family, *kinds = ROLE_SETS[(0, 6, 7, 8, 3)[j]]
        out[f"segments-{name}-{family}"] = make_case(
            200 + j, family, [k for k in kinds if k], 5, N, 2 * len(lengths), index,
            shift=TERMS[j % 3], mult=TERMS[(j + 1) % 3], mask=("none", "random")[j % 2],
            int_values=True)
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
def test_gather_site_against_reference(name):
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
    for key, value in got.items():
        if value.ndim == 2:
            assert np.all(value[:, ~present] == 0.0), key
    rc2, again, _ = launch(case, device)
    assert rc2 == 0
    for key in got:   # bit for bit
        assert np.array_equal(got[key].view(np.uint32), again[key].view(np.uint32)), key


def _flag_case(family, bad, masked):
    N, K, G = 70, 5, 3
    rng = np.random.default_rng(7)
    kinds = {"normal": ["g", "p"], "bernoulli": ["g"], "poisson": ["g"]}[family]
    case = make_case(300, family, kinds, K, N, G, make_index(rng, "random", N, G))
    row = 37
    if bad == "support":
        case["value"][row] = {"normal": np.nan, "bernoulli": 0.5, "poisson": 1.5}[family]
    elif bad == "negative":
        case["value"][row] = -1.0
    elif bad == "eta":
        case["roles"][0][1][2, case["index"][row]] = np.inf
        case["index"][:] = np.where(np.arange(N) == row, case["index"][row],
                                    (case["index"][row] + 1) % G)   # the group has that row only
    else:   # a scale that is not positive
        case["roles"][1][1][3] = 0.0 if bad == "scale0" else -1.0
    mask = np.ones(N, bool)
    if masked:
        # every row whose parameter is invalid is masked out (a per-particle scale: all rows)
        mask[:] = bad not in ("scale0", "scale-")
        mask[row] = False
    case["mask"] = mask
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("family, bad, bit", [
    ("normal", "support", nat.FLAG_SUPPORT), ("bernoulli", "support", nat.FLAG_SUPPORT),
    ("poisson", "support", nat.FLAG_SUPPORT), ("poisson", "negative", nat.FLAG_SUPPORT),
    ("normal", "eta", nat.FLAG_PARAM), ("bernoulli", "eta", nat.FLAG_PARAM),
    ("poisson", "eta", nat.FLAG_PARAM), ("normal", "scale0", nat.FLAG_PARAM),
    ("normal", "scale-", nat.FLAG_PARAM)])
def test_flags_on_observed_rows_only(family, bad, bit):
    device = torch.device("cuda")
    rc, _, flags = launch(_flag_case(family, bad, False), device)
    assert rc == 0 and flags == bit, (rc, flags)
    rc, got, flags = launch(_flag_case(family, bad, True), device)
    assert rc == 0 and flags == 0, (rc, flags)
    assert np.isfinite(got["total"]).all()


@pytest.mark.gpu
def test_group_outside_the_table_is_never_an_address():
    """Entries of sorted_group outside [0, G) add nothing and set MI_FLAG_INTERNAL; the table is a
    buffer of exactly K * G floats between guard bands of the launch's own allocations."""
    rng = np.random.default_rng(11)
    N, K, G = 300, 5, 4
    case = make_case(400, "normal", ["g", "p"], K, N, G, np.sort(rng.integers(0, G, N)))
    sg = np.sort(case["index"]).astype(np.int32)
    sg[:2] = -5
    sg[-3:] = G + 1000000
    rc, got, flags = launch(case, torch.device("cuda"), sorted_group=sg)
    assert rc == 0 and flags == nat.FLAG_INTERNAL
    # the same site with those rows masked out
    mask = np.ones(N, bool)
    order = np.argsort(case["index"], kind="stable")
    mask[order[:2]] = False
    mask[order[-3:]] = False
    check(dict(case, mask=mask), {"total": got["total"]})
