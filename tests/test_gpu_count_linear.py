"""
The count regressions of the linear-predictor site kernels (csrc/linear.hip: MI_POISSON with the log
link, MI_BINOMIAL, MI_NEGATIVE_BINOMIAL) point by point against the fp64 reference of
tests/count_linear_reference.py, through the C ABI and over poisoned buffers, in the pattern of
test_gpu_linear_variants.py: every case first asserts its launch variant from geometry().

Tolerances (the project's own): gradients 1e-5 of g0 x the sum of |terms| (+ 1e-7); totals 1e-5 of
the sum over rows of the absolute values of the log density's separate parts (Poisson: |y eta|,
exp(eta), |lgamma(y + 1)|), and in the plain regime (|eta| <= 3) also 1e-5 relative to the total.
test_count_linear_host.py holds a float32 restatement of the kernels' formula to both bounds on
these inputs without a GPU.
"""
import dataclasses
import functools
import zlib
from typing import Optional

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests.count_linear_reference import launch, reference
from tests.linear_reference import Prior, geometry

pytestmark = pytest.mark.gpu

PO, BI, NB = nat.POISSON, nat.BINOMIAL, nat.NEGATIVE_BINOMIAL
NAMES = {PO: "poisson", BI: "binomial", NB: "negbinomial"}
SITE_SCALE = 3.0
PRIOR = Prior(nat.NORMAL, 0.3, 1.5, 0.7)   # prior.scale != site_scale


@dataclasses.dataclass(frozen=True)
class Case:
    family: int
    N: int
    P: int
    K: int
    masked: bool = False
    rows: bool = False               # row_index: a permutation with repeats into a larger dataset
    prior: bool = False
    regime: str = "plain"            # plain, eta-20, eta8, logit20, logit90, point
    strided: bool = False            # value, mask and count with stride 3
    theta_slice: bool = False
    count: str = "rows"              # rows: per-row array; constant: the host constant
    expect: tuple = ()

    @property
    def id(self):
        parts = [NAMES[self.family], f"N{self.N}_P{self.P}_K{self.K}"]
        parts += [w for w, on in (("masked", self.masked), ("rows", self.rows),
                                  ("strided", self.strided), ("slice", self.theta_slice),
                                  ("prior", self.prior)) if on]
        parts += [w for w in (self.regime, self.count) if w not in ("plain", "rows")]
        return "-".join(parts)

    @property
    def eligible(self):
        return self.P % 4 == 0

    def geometry(self, valu=False):
        return geometry(self.N, self.P, self.K, False, self.prior, self.eligible and not valu)

    def check_variant(self, valu=False):
        g = self.geometry(valu)
        assert g.nv == 1 + self.P
        assert g.mfma == (self.eligible and not valu)
        if not valu:
            for name, want in self.expect:
                assert getattr(g, name) == want, (self.id, name, getattr(g, name), want)
        return g


def ex(**kw):
    return tuple(sorted(kw.items()))


def three(expect, N, P, K, **kw):
    return [Case(f, N, P, K, expect=expect, **kw) for f in (PO, BI, NB)]


# the geometries of test_gpu_linear_variants.py
MS_A = ex(mfma=True, pt=1, wt=4, gy=64, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1,
          combine=False, ntile=16)
MS_B = ex(mfma=True, pt=2, wt=4, gy=64, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1,
          combine=False, ntile=16)
MS_D = ex(mfma=True, pt=1, wt=2, row_subsets=2, stages_per_block=2, combine=True, ntile=552,
          chunked_finalize=True)
ONE = ex(mfma=True, stages_per_block=1)
MS_A_PRIOR = ex(mfma=True, pt=1, stages_per_block=2, ntile=17)

MULTI_STAGE = (three(MS_A, 2177, 32, 8161, masked=True) +
               three(MS_A, 2177, 32, 8161, masked=True, rows=True) +
               three(MS_B, 1089, 40, 8161) +
               three(MS_D, 140000, 32, 33, masked=True))
ONE_STAGE = (three(ONE, 1, 4, 1) + three(ONE, 33, 4, 33) + three(ONE, 129, 32, 31, masked=True) +
             three(ONE, 777, 32, 40, masked=True, strided=True, theta_slice=True) +
             three(ONE, 300, 60, 33, masked=True, rows=True))
VALU_ONLY = [c for P in (3, 5) for c in three(ex(mfma=False), 1000, P, 300, masked=True) +
             three(ex(mfma=False), 65, P, 31, rows=True)]
CROSS = three(ONE, 1000, 32, 256, masked=True)      # MI_LINEAR_VALU on an MFMA-eligible case
NO_GRADS = three(MS_A, 2177, 32, 8161, masked=True) + three(ONE, 777, 32, 40, masked=True)
FOLDED = three(ONE, 777, 32, 40, masked=True, prior=True) + \
    [Case(PO, 2177, 32, 8161, masked=True, prior=True, expect=MS_A_PRIOR)]
# (N, K, expect, VALU kernel): the three paths
PATHS = {"onestage": (777, 40, ONE, False), "multistage": (2177, 8161, MS_A, False),
         "valu": (777, 40, ONE, True)}
REGIMES = [(Case(f, N, 32, K, masked=N == 2177, regime=regime, expect=expect), valu)
           for f, regimes in ((PO, ("eta-20", "eta8")), (BI, ("logit20", "logit90")),
                              (NB, ("logit20", "logit90", "point")))
           for regime in regimes for N, K, expect, valu in PATHS.values()]
CONSTANT = [Case(f, 777, 32, 40, masked=True, count="constant", expect=ONE) for f in (BI, NB)]

ALL_CASES = ([(c, False) for c in MULTI_STAGE + ONE_STAGE + VALU_ONLY + FOLDED + CONSTANT] +
             [(c, valu) for c in CROSS + NO_GRADS for valu in (False, True)] + REGIMES +
             [(Case(f, N, 32, K, expect=expect), valu) for f in (PO, BI, NB)
              for N, K, expect, valu in PATHS.values()])


# ---- inputs ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def inputs(case):
    """The case's arrays, in numpy: X [D, P] (the dataset), theta, y, mask, count, row_index."""
    key = dataclasses.replace(case, expect=(), strided=False, theta_slice=False)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    N, P, K = case.N, case.P, case.K
    D = N + N // 2 + 3 if case.rows else N
    X = rng.normal(size=(D, P)).astype(np.float32)
    u = rng.normal(size=P)
    u /= np.linalg.norm(u)
    if case.regime in ("eta-20", "eta8"):
        # an intercept column; the other features move eta by a few tenths
        X[:, 0] = 1.0
        theta = 0.1 * rng.normal(size=(K, P)) / np.sqrt(P)
        theta[:, 0] = -20.0 if case.regime == "eta-20" else rng.uniform(4.0, 7.5, size=K)
    elif case.regime.startswith("logit"):
        M = float(case.regime[5:])
        theta = M * (u[None, :] + 0.1 * rng.normal(size=(K, P)) / np.sqrt(P))
    else:
        # |eta| <= 3 (six standard deviations of eta: the plain regime)
        theta = 0.5 * rng.normal(size=(K, P)) / np.sqrt(P)
        theta *= min(1.0, 2.9 / np.abs(X.astype(np.float64) @ theta.T).max())
    theta = theta.astype(np.float32)
    direction = X.astype(np.float64) @ u
    if case.family == BI:
        count = rng.integers(1, 21, size=D).astype(np.float32)
    else:
        count = rng.choice([0.5, 1.0, 2.5, 7.0], size=D).astype(np.float32)
    if case.count == "constant":
        count[:] = 6.0
    if case.regime == "eta-20":
        y = np.zeros(D, np.float32)
    elif case.regime == "eta8":
        y = rng.poisson(np.exp(X.astype(np.float64) @ theta[0].astype(np.float64))).astype(np.float32)
    elif case.family == PO:
        y = rng.poisson(np.exp(0.5 * direction)).astype(np.float32)
    elif case.family == BI and case.regime.startswith("logit"):
        # y sides with the sign of the logit in 70% of the rows
        agree = rng.random(D) < 0.7
        y = np.where((direction > 0) == agree, count, 0.0).astype(np.float32)
    elif case.family == BI:
        y = rng.binomial(count.astype(np.int64), 0.4).astype(np.float32)
    else:
        y = rng.poisson(3.0, size=D).astype(np.float32)
        if case.regime == "point":
            point = rng.random(D) < 0.2           # rows with r + y == 0: probability 1
            y[point], count[point] = 0.0, 0.0
    mask = rng.random(D) > 0.15 if case.masked else np.ones(D, bool)
    if case.masked:
        y[~mask] = 0.5                            # masked lanes are never read
        count[~mask] = -1.5
    rows = None
    if case.rows:
        rows = rng.permutation(D)[:N].astype(np.int32)
        rows[N // 2:N // 2 + N // 10] = rows[:N // 10]
    return dict(X=X, theta=theta, y=y, mask=mask, count=count, rows=rows)


@functools.lru_cache(maxsize=None)
def reference_of(case):
    a = inputs(case)
    return reference(case.family, a["X"], a["theta"], a["y"], a["mask"], a["count"], SITE_SCALE,
                     -1.0 / case.K, row_index=a["rows"], prior=PRIOR if case.prior else None)


def strided3(array, device):
    store = torch.zeros(3 * len(array), dtype=torch.as_tensor(array).dtype, device=device)
    store[::3] = torch.as_tensor(array, device=device)
    return store[::3]


def upload(case, a, device):
    Xd = torch.as_tensor(a["X"], device=device)
    P = case.P
    if case.theta_slice:
        wide = torch.full((case.K, P + 8), float("nan"), device=device)
        wide[:, 3:3 + P] = torch.as_tensor(a["theta"], device=device)
        theta = wide[:, 3:3 + P]
    else:
        theta = torch.as_tensor(a["theta"], device=device)
    put = (lambda v: strided3(v, device)) if case.strided else \
        (lambda v: torch.as_tensor(v, device=device))
    y = put(a["y"])
    mask = put(a["mask"].astype(np.uint8)) if case.masked else None
    if case.family == PO:
        count = None
    elif case.count == "constant":
        count = float(a["count"][a["mask"]][0])
    else:
        count = put(a["count"])
    rows = None if a["rows"] is None else torch.as_tensor(a["rows"], device=device)
    return Xd, theta, y, mask, count, rows


def launch_case(case, device, valu=False, compute_grads=1, arrays=None, count=None):
    g = case.check_variant(valu)
    a = arrays if arrays is not None else inputs(case)
    X, theta, y, mask, cnt, rows = upload(case, a, device)
    r = launch(case.family, X, theta, y, mask, cnt if count is None else count, SITE_SCALE,
               -1.0 / case.K, valu, compute_grads=compute_grads, row_index=rows,
               prior=PRIOR if case.prior else None)
    assert vars(r.geometry) == vars(g)
    return r


def compare(case, r, grads=True):
    """The launch against fp64; prints the largest error as a fraction of its bound."""
    assert r.rc == 0
    assert r.flags == 0, r.flags
    if case.prior:
        assert r.prior_flags == 0, r.prior_flags
    want, dtheta, bound, tbound = reference_of(case)
    g0 = 1.0 / case.K
    assert np.isfinite(r.total).all()
    terr = np.abs(r.total - want)
    fractions = {"total_parts": (terr / (1e-5 * tbound)).max()}
    if case.regime == "plain":
        fractions["total"] = (terr / (1e-5 * np.abs(want))).max()
    if grads:
        assert np.isfinite(r.dslots).all()
        err = np.abs(r.dslots.T - dtheta)
        fractions["dtheta"] = (err / (1e-5 * g0 * bound + 1e-7)).max()
    print("ERRFRAC", case.id, " ".join(f"{k}={v:.3f}" for k, v in fractions.items()))
    assert (terr <= 1e-5 * tbound).all(), fractions
    if case.regime == "plain":
        assert (terr <= 1e-5 * np.abs(want)).all(), fractions
    if grads:
        assert (err <= 1e-5 * g0 * bound + 1e-7).all(), fractions
    return fractions


def ids(cases):
    return [c.id if isinstance(c, Case) else c[0].id + ("-valu" if c[1] else "") for c in cases]


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda")


@pytest.mark.parametrize("case", MULTI_STAGE + ONE_STAGE + VALU_ONLY + FOLDED, ids=ids(
    MULTI_STAGE + ONE_STAGE + VALU_ONLY + FOLDED))
def test_variant_against_fp64(case, device):
    compare(case, launch_case(case, device))


@pytest.mark.parametrize("case,valu", REGIMES, ids=ids(REGIMES))
def test_regimes(case, valu, device):
    compare(case, launch_case(case, device, valu=valu))


@pytest.mark.parametrize("case", CROSS, ids=ids(CROSS))
def test_valu_option_agrees_with_the_matrix_cores(case, device):
    mf = launch_case(case, device)
    va = launch_case(case, device, valu=True)
    compare(case, mf)
    compare(case, va)
    _, _, _, tbound = reference_of(case)
    assert (np.abs(mf.total - va.total) <= 1e-5 * tbound).all()


@pytest.mark.parametrize("case", NO_GRADS, ids=ids(NO_GRADS))
@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
def test_no_grads_totals_bit_equal(case, valu, device):
    with_grads = launch_case(case, device, valu=valu)
    without = launch_case(case, device, valu=valu, compute_grads=0)   # (asserts dslots untouched)
    assert without.rc == 0 and without.flags == 0
    assert np.array_equal(with_grads.total, without.total)
    compare(case, without, grads=False)


@pytest.mark.parametrize("case", CONSTANT, ids=ids(CONSTANT))
def test_constant_count_equals_equal_rows(case, device):
    a = inputs(case)
    constant = launch_case(case, device)
    per_row = launch_case(case, device, count=torch.as_tensor(
        np.where(a["mask"], a["count"], 6.0).astype(np.float32), device=device))
    compare(case, constant)
    assert np.array_equal(constant.total, per_row.total)
    assert np.array_equal(constant.dslots, per_row.dslots)


# ---- flags ------------------------------------------------------------------------------------------
def flag_case(family, path):
    N, K, expect, valu = PATHS[path]
    return Case(family, N, 32, K, expect=expect), valu


def with_bad(case, **changes):
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inputs(case).items()}
    for key, (index, value) in changes.items():
        a[key][index] = value
    return a


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("family", [PO, BI, NB], ids=list(NAMES.values()))
def test_flags(family, path, device):
    case, valu = flag_case(family, path)
    row = case.N - 3
    assert launch_case(case, device, valu=valu).flags == 0
    bad_values = [0.5, -1.0] + ([25.0] if family == BI else [])   # 25 > every n_i
    for bad in bad_values:
        r = launch_case(case, device, valu=valu, arrays=with_bad(case, y=(row, bad)))
        assert r.rc == 0 and r.flags == nat.FLAG_SUPPORT, (bad, r.flags)
    # the same value under a masked-out row raises nothing
    masked = dataclasses.replace(case, masked=True)
    a = with_bad(masked, y=(row, -1.0), mask=(row, False))
    r = launch_case(masked, device, valu=valu, arrays=a)
    assert r.rc == 0 and r.flags == 0, r.flags
    r = launch_case(case, device, valu=valu,
                    arrays=with_bad(case, theta=((case.K - 1, 5), float("nan"))))
    assert r.rc == 0 and r.flags == nat.FLAG_PARAM, r.flags
    if family != PO:
        r = launch_case(case, device, valu=valu, arrays=with_bad(case, count=(row, -2.0)))
        assert r.rc == 0 and r.flags & nat.FLAG_PARAM, r.flags
    if family == BI:
        r = launch_case(case, device, valu=valu, arrays=with_bad(case, count=(row, 30.5)))
        assert r.rc == 0 and r.flags == nat.FLAG_PARAM, r.flags
