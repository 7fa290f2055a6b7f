"""
Every launch variant of the linear-predictor site kernels (csrc/linear.hip) point by point against
the fp64 reference of tests/linear_reference.py, through the C ABI and over poisoned buffers:

* the multi-stage matrix-core kernel (register prefetch, software pipeline over tiles, dtheta
  carried in fp32 over the block's rows), one and two feature tiles, row blocks without a stage, a
  ragged last stage, row subsets combined in LDS, the chunked finalize, row_index and strided rows;
* compute_grads = 0 on every kernel: totals bit-equal to the launch with gradients, dslots untouched;
* the VALU kernel where it is the only choice: P % 4 != 0 and the three fall-back conditions;
* one-stage edges in N and K, strided value / mask / sigma and a theta that is a column slice;
* the folded prior (Normal, Beta, Gamma; prior.scale != site_scale) in both spellings of its loop;
* Bernoulli logits of magnitude 20, 90 and 200, Normal sigma of 1e-3, 1e-2 and 30;
* the flag words on all three paths.

Every case first asserts from geometry() the variant it is named for (CASE.expect), so a retuning
of the launch constants fails the case instead of moving it to another kernel; the same asserts
and the byte count of geometry() against the library run without a GPU in
test_linear_geometry_host.py.

Tolerances (the north-star ELBO tolerance, as test_gpu_linear.py): totals 1e-5 relative, per
particle; gradients 1e-5 of the sum of |terms| (+ 1e-7).
"""
import dataclasses
import functools
import zlib
from typing import Optional

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests.linear_reference import Prior, geometry, launch, prior_terms, reference

pytestmark = pytest.mark.gpu

N_, B_ = nat.NORMAL, nat.BERNOULLI_LOGITS
SITE_SCALE = 3.0
PRIOR_SCALE = 0.7
PRIORS = {"normal": Prior(nat.NORMAL, 0.3, 1.5, PRIOR_SCALE),
          "beta": Prior(nat.BETA, 2.0, 3.0, PRIOR_SCALE),
          "gamma": Prior(nat.GAMMA, 2.0, 3.0, PRIOR_SCALE)}


@dataclasses.dataclass(frozen=True)
class Case:
    family: int
    N: int
    P: int
    K: int
    masked: bool = False
    per_particle: bool = False       # Normal: a sigma per particle
    layout: str = "dense"            # X: dense, stride40, stride33, offset1, transposed
    rows: bool = False               # row_index: a permutation with repeats into a larger dataset
    prior: Optional[str] = None      # key of PRIORS
    regime: str = "plain"            # plain, logit20, logit90, logit200, sigma_mixed, sigma_small
    strided: bool = False            # value, mask and sigma with stride 3
    theta_slice: bool = False        # theta a column slice of a wider matrix
    expect: tuple = ()               # (attribute of geometry(), value) pairs: the variant

    @property
    def id(self):
        parts = ["normal" if self.family == N_ else "bernoulli", f"N{self.N}_P{self.P}_K{self.K}"]
        parts += [w for w, on in (("masked", self.masked), ("sigmak", self.per_particle),
                                  ("rows", self.rows), ("strided", self.strided),
                                  ("slice", self.theta_slice)) if on]
        parts += [w for w in (self.layout, self.regime) if w not in ("dense", "plain")]
        if self.prior:
            parts.append("prior_" + self.prior)
        return "-".join(parts)

    @property
    def eligible(self):
        """The inputs meet the matrix-core kernel's conditions (use_mfma() of linear.hip)."""
        return self.P % 4 == 0 and self.layout in ("dense", "stride40")

    def geometry(self, valu=False):
        return geometry(self.N, self.P, self.K, self.per_particle and self.family == N_,
                        self.prior is not None, self.eligible and not valu)

    def check_variant(self, valu=False):
        g = self.geometry(valu)
        assert g.mfma == (self.eligible and not valu)
        if not valu:
            for name, want in self.expect:
                assert getattr(g, name) == want, (self.id, name, getattr(g, name), want)
        return g


def both(expect, N, P, K, normal=None, bernoulli=None, **common):
    """The case in both families (per-particle sigma is the Normal one's)."""
    nk = dict(common, **(normal or {}))
    bk = dict(common, **(bernoulli or {}))
    bk.pop("per_particle", None)
    return [Case(N_, N, P, K, expect=expect, **nk), Case(B_, N, P, K, expect=expect, **bk)]


def ex(**kw):
    return tuple(sorted(kw.items()))


# ---- the multi-stage matrix-core kernel ---------------------------------------------------------
# 256 threads, 128 / PT rows per stage, 1024 / gy blocks aimed at: see geometry().
MS_A = ex(mfma=True, pt=1, wt=4, gy=64, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1,
          combine=False, ntile=16)
MS_B = ex(mfma=True, pt=2, wt=4, gy=64, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1,
          combine=False, ntile=16)
MS_C = ex(mfma=True, pt=1, gy=64, stages_per_block=3, last_block_stages=1, last_stage_rows=8,
          empty_row_blocks=2, combine=False)
MS_D = ex(mfma=True, pt=1, wt=2, row_subsets=2, stages_per_block=2, combine=True, ntile=552,
          chunked_finalize=True)
MS_E = ex(mfma=True, pt=2, wt=2, row_subsets=2, stages_per_block=2, combine=True,
          combine_floats=4352, lds_floats=4352, ntile=552, chunked_finalize=True)
MS_F = ex(mfma=True, pt=2, wt=2, stages_per_block=3, combine=True, chunked_finalize=True)
MS_G = ex(mfma=True, pt=1, wt=1, row_subsets=4, stages_per_block=3, combine=True,
          chunked_finalize=True)

MULTI_STAGE = (
    both(MS_A, 2177, 32, 8161, masked=True, per_particle=True) +
    both(MS_B, 1089, 40, 8161, per_particle=True) +
    both(MS_C, 5000, 32, 8161) +
    both(MS_D, 140000, 32, 33, masked=True) +
    both(MS_E, 70000, 36, 40, per_particle=True) +
    both(MS_F, 140000, 64, 64) +
    both(MS_G, 300000, 32, 1) +
    [Case(N_, 2177, 32, 8161, masked=True, per_particle=True, rows=True, expect=MS_A),
     Case(B_, 140000, 32, 33, masked=True, rows=True, expect=MS_D),
     Case(N_, 5000, 32, 8161, layout="stride40", expect=MS_C),
     Case(B_, 1089, 40, 8161, layout="stride40", rows=True, expect=MS_B)])

# ---- compute_grads = 0 ----------------------------------------------------------------------------
ONE = ex(mfma=True, stages_per_block=1)
NO_GRADS = (
    both(MS_A, 2177, 32, 8161, masked=True, per_particle=True) +
    both(MS_D, 140000, 32, 33, masked=True) +
    both(ONE, 1000, 32, 256) +
    both(ONE, 777, 32, 40, masked=True, per_particle=True))

# ---- the VALU kernel where it is the only choice ------------------------------------------------
VALU_P = (1, 3, 5, 13, 17, 33, 63)
VALU_K = (1, 31, 257, 300)
VALU_N = (1, 63, 64, 65, 1000)
VALU_ONLY = {(f, P): [Case(f, N, P, K, masked=N > 1, per_particle=True if f == N_ else False,
                           expect=ex(mfma=False))
                      for K in VALU_K for N in VALU_N]
             for f in (N_, B_) for P in VALU_P}
FALLBACK = [c for layout in ("stride33", "offset1", "transposed")
            for c in both(ex(mfma=False), 1000, 32, 40, masked=True, per_particle=True,
                          layout=layout)]

# ---- one-stage edges ----------------------------------------------------------------------------
ONE_NC = ex(mfma=True, stages_per_block=1, pt=2, wt=1, row_subsets=4, combine=False, ntile=32)
ONE_STAGE = (
    [c for N in (1, 31, 32, 33, 127, 128, 129)
     for c in both(ONE, N, 32, 40, masked=N > 1, per_particle=True)] +
    # two feature tiles, one particle tile: four row subsets that do not fit the LDS combine
    [c for N in (63, 64, 65) for c in both(ONE_NC, N, 64, 20, masked=True, per_particle=True)] +
    [c for K in (1, 32, 33) for c in both(ONE, 300, 32, K, per_particle=True)] +
    # a second particle group with three waves entirely past K
    both(ex(mfma=True, stages_per_block=1, wt=4, gy=2), 300, 32, 129, per_particle=True) +
    both(ONE, 777, 32, 40, masked=True, per_particle=True, strided=True, theta_slice=True) +
    both(ONE, 300, 60, 33, masked=True, per_particle=True, strided=True, theta_slice=True))

# ---- the folded prior ---------------------------------------------------------------------------
ONE_P1 = ex(mfma=True, stages_per_block=1, pt=1)
ONE_P2 = ex(mfma=True, stages_per_block=1, pt=2)
MS_A_PRIOR = ex(mfma=True, pt=1, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1, ntile=17)
MS_B_PRIOR = ex(mfma=True, pt=2, stages_per_block=2, empty_row_blocks=7, last_stage_rows=1, ntile=17)
FOLDED_PRIOR = [c for prior in PRIORS for c in (
    both(ONE_P1, 777, 32, 40, masked=True, per_particle=True, prior=prior) +
    [Case(N_, 300, 60, 33, per_particle=True, prior=prior, expect=ONE_P2)] +
    both(MS_A_PRIOR, 2177, 32, 8161, masked=True, per_particle=True, prior=prior) +
    [Case(N_, 1089, 40, 8161, per_particle=True, prior=prior, expect=MS_B_PRIOR),
     Case(N_, 1089, 60, 8161, per_particle=True, prior=prior, expect=MS_B_PRIOR)])]

# ---- extreme regimes ----------------------------------------------------------------------------
# (case, VALU kernel): the one-stage and the multi-stage matrix-core kernel and the VALU kernel
EXTREME = (
    [(Case(B_, N, 32, K, masked=N == 2177, regime=regime, expect=expect), valu)
     for regime in ("logit20", "logit90", "logit200")
     for N, K, expect, valu in ((1000, 256, ONE, False), (2177, 8161, MS_A, False),
                                (1000, 256, ONE, True))] +
    [(Case(N_, N, 32, K, masked=N == 2177, per_particle=regime == "sigma_mixed", regime=regime,
           expect=expect), valu)
     for regime in ("sigma_mixed", "sigma_small")
     for N, K, expect, valu in ((1000, 256, ONE, False), (2177, 8161, MS_A, False),
                                (1000, 256, ONE, True))])

# ---- the three paths of the flag tests ------------------------------------------------------------
PATHS = {"onestage": (777, 40, ONE, False), "multistage": (2177, 8161, MS_A, False),
         "valu": (777, 40, ONE, True)}

# every case above with the kernel choice it runs under, for test_linear_geometry_host.py
ALL_CASES = (
    [(c, False) for c in MULTI_STAGE] +
    [(c, valu) for c in NO_GRADS for valu in (False, True)] +
    [(c, False) for cases in VALU_ONLY.values() for c in cases] +
    [(c, False) for c in FALLBACK + ONE_STAGE + FOLDED_PRIOR] +
    EXTREME +
    [(Case(N_, N, 32, K, per_particle=True, expect=expect), valu)
     for N, K, expect, valu in PATHS.values()])


# ---- inputs ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def inputs(case):
    """The case's arrays, in numpy: X [D, P] (the dataset), theta, y, mask, sigma, row_index."""
    key = dataclasses.replace(case, expect=(), layout="dense", strided=False, theta_slice=False)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    N, P, K = case.N, case.P, case.K
    D = N + N // 2 + 3 if case.rows else N
    X = rng.normal(size=(D, P)).astype(np.float32)
    if case.prior == "beta":
        theta = rng.uniform(0.05, 0.95, size=(K, P))
    elif case.prior == "gamma":
        theta = rng.uniform(0.1, 2.0, size=(K, P))
    elif case.regime.startswith("logit"):
        # logits of typical magnitude M, their sign shared by the particles
        M = float(case.regime[5:])
        u = rng.normal(size=P)
        u /= np.linalg.norm(u)
        theta = M * (u[None, :] + 0.1 * rng.normal(size=(K, P)) / np.sqrt(P))
    else:
        theta = 0.3 * rng.normal(size=(K, P))
    theta = theta.astype(np.float32)
    if case.family == N_:
        y = rng.normal(size=D).astype(np.float32)
    elif case.regime.startswith("logit"):
        # y agrees with the sign of the logit in 70% of the rows and disagrees in the rest
        agree = rng.random(D) < 0.7
        y = ((X.astype(np.float64) @ u > 0) == agree).astype(np.float32)
    else:
        y = (rng.random(D) < 0.4).astype(np.float32)
    mask = rng.random(D) > 0.15 if case.masked else np.ones(D, bool)
    if case.masked:
        y[~mask] = np.nan if case.family == N_ else 0.5   # masked lanes are never read
    if case.regime == "sigma_mixed":
        sigma = np.where(np.arange(K) % 2 == 0, 1e-3, 30.0).astype(np.float32)
    elif case.regime == "sigma_small":
        sigma = np.full(K, 1e-2, np.float32)
    elif case.per_particle:
        sigma = (0.5 + rng.random(K)).astype(np.float32)
    else:
        sigma = np.full(K, 0.8, np.float32)
    rows = None
    if case.rows:
        rows = rng.permutation(D)[:N].astype(np.int32)
        rows[N // 2:N // 2 + N // 10] = rows[:N // 10]    # repeated rows
    return dict(X=X, theta=theta, y=y, mask=mask, sigma=sigma, rows=rows)


@functools.lru_cache(maxsize=None)
def reference_of(case):
    a = inputs(case)
    g0 = -1.0 / case.K
    return reference(case.family, a["X"], a["theta"], a["y"], a["mask"], a["sigma"], SITE_SCALE, g0,
                     row_index=a["rows"], prior=PRIORS[case.prior] if case.prior else None)


def strided3(array, device):
    store = torch.zeros(3 * len(array), dtype=torch.as_tensor(array).dtype, device=device)
    store[::3] = torch.as_tensor(array, device=device)
    return store[::3]


def upload(case, a, device):
    """Device tensors of the arrays in the case's layout."""
    X, (D, P) = a["X"], a["X"].shape
    if case.layout in ("stride40", "stride33"):
        stride = int(case.layout[6:])
        wide = torch.full((D, stride), float("nan"), device=device)   # the padding is never read
        wide[:, :P] = torch.as_tensor(X, device=device)
        Xd = wide[:, :P]
    elif case.layout == "offset1":
        flat = torch.empty(D * P + 4, device=device)
        Xd = flat[1:1 + D * P].view(D, P)
        Xd.copy_(torch.as_tensor(X, device=device))
        assert Xd.data_ptr() % 16 == 4
    elif case.layout == "transposed":
        Xd = torch.as_tensor(np.ascontiguousarray(X.T), device=device).t()
        assert Xd.stride(1) != 1
    else:
        Xd = torch.as_tensor(X, device=device)
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
    sigma = put(a["sigma"])
    rows = None if a["rows"] is None else torch.as_tensor(a["rows"], device=device)
    return Xd, theta, y, mask, sigma, rows


def launch_case(case, device, valu=False, compute_grads=1, arrays=None, flags_zeroed=False):
    g = case.check_variant(valu)
    a = arrays if arrays is not None else inputs(case)
    X, theta, y, mask, sigma, rows = upload(case, a, device)
    per_particle = case.per_particle and case.family == N_
    r = launch(case.family, X, theta, y, mask, sigma, per_particle, SITE_SCALE, -1.0 / case.K, valu,
               compute_grads=compute_grads, row_index=rows,
               prior=PRIORS[case.prior] if case.prior else None, flags_zeroed=flags_zeroed)
    # launch() holds the library's workspace size to geometry(): the launch is the variant asserted
    assert vars(r.geometry) == vars(g)
    return r


def compare(case, r, grads=True):
    """The launch against fp64; prints the largest error as a fraction of its bound."""
    assert r.rc == 0
    assert r.flags == 0, r.flags          # (over a poisoned word: the launch cleared it)
    if case.prior:
        assert r.prior_flags == 0, r.prior_flags
    want, dtheta, dsigma, bound, sbound = reference_of(case)
    g0, P = 1.0 / case.K, case.P
    assert np.isfinite(r.total).all()
    terr = np.abs(r.total - want)
    fractions = {"total": (terr / (1e-5 * np.abs(want))).max()}
    if grads:
        assert np.isfinite(r.dslots).all()
        err = np.abs(r.dslots[:P].T - dtheta)
        fractions["dtheta"] = (err / (1e-5 * g0 * bound + 1e-7)).max()
        if case.per_particle and case.family == N_:
            serr = np.abs(r.dslots[P] - dsigma)
            fractions["dsigma"] = (serr / (1e-5 * g0 * sbound + 1e-7)).max()
    print("ERRFRAC", case.id, " ".join(f"{k}={v:.3f}" for k, v in fractions.items()))
    assert (terr <= 1e-5 * np.abs(want)).all(), fractions
    if grads:
        assert (err <= 1e-5 * g0 * bound + 1e-7).all(), fractions
        if "dsigma" in fractions:
            assert (serr <= 1e-5 * g0 * sbound + 1e-7).all(), fractions
    return fractions


def ids(cases):
    return [c.id for c in cases]


# ---- tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MULTI_STAGE, ids=ids(MULTI_STAGE))
def test_multi_stage_kernel_matches_fp64(device, case):
    assert case.geometry().stages_per_block >= 2
    compare(case, launch_case(case, device))


@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
@pytest.mark.parametrize("case", NO_GRADS, ids=ids(NO_GRADS))
def test_values_only_launch(device, case, valu):
    """compute_grads = 0: the GRADS = false kernels. launch() checks that dslots stays NaN."""
    with_grads = launch_case(case, device, valu)
    values_only = launch_case(case, device, valu, compute_grads=0)
    compare(case, values_only, grads=False)
    # the value arithmetic does not depend on GRADS
    assert np.array_equal(values_only.total, with_grads.total)


@pytest.mark.parametrize("key", list(VALU_ONLY),
                         ids=[("normal" if f == N_ else "bernoulli") + f"_P{P}" for f, P in VALU_ONLY])
def test_valu_kernel_feature_padding(device, key):
    """P % 4 != 0: the VALU kernel with the P it exists for (j < P padding inside PMAX)."""
    worst = {}
    for case in VALU_ONLY[key]:
        assert not case.geometry().mfma
        for name, value in compare(case, launch_case(case, device)).items():
            worst[name] = max(worst.get(name, 0.0), value)
    print("ERRFRAC-WORST", key, worst)


@pytest.mark.parametrize("case", FALLBACK, ids=ids(FALLBACK))
def test_valu_kernel_fallback_conditions(device, case):
    """Inputs the matrix-core kernel does not take: the launch must fall back, and be right."""
    assert not case.geometry().mfma and case.P % 4 == 0
    compare(case, launch_case(case, device))


@pytest.mark.parametrize("case", ONE_STAGE, ids=ids(ONE_STAGE))
def test_one_stage_edges(device, case):
    assert case.geometry().stages_per_block == 1
    compare(case, launch_case(case, device))


@pytest.mark.parametrize("case", FOLDED_PRIOR, ids=ids(FOLDED_PRIOR))
def test_folded_prior_matches_fp64(device, case):
    """The prior's terms in the total and dtheta; dsigma is the likelihood's alone."""
    r = launch_case(case, device)
    compare(case, r)
    # the prior's share is well above the tolerance: a launch without it would not pass
    plp, pd = prior_terms(PRIORS[case.prior], inputs(case)["theta"].astype(np.float64))
    want, _, _, bound, _ = reference_of(case)
    assert (np.abs(PRIOR_SCALE * plp.sum(1)) > 1e-5 * np.abs(want)).mean() > 0.5
    assert (np.abs(PRIOR_SCALE * pd) > 1e-5 * bound).mean() > 0.5


@pytest.mark.parametrize("path", list(PATHS))
def test_folded_prior_flags(device, path):
    N, K, expect, valu = PATHS[path]
    expect = tuple(e for e in expect if e[0] != "ntile")   # (the prior's tile is one more)
    case = Case(N_, N, 32, K, per_particle=True, prior="beta", expect=expect)
    a = dict(inputs(case))
    if valu:   # the VALU kernel has no folded prior
        r = launch_case(dataclasses.replace(case, expect=()), device, valu=True)
        assert r.rc == nat.MI_EUNSUPPORTED
        assert np.isnan(r.total).all()
        return
    # a theta outside the prior's support is the prior's violation alone
    a["theta"] = a["theta"].copy()
    a["theta"][K - 1, 5] = 1.5
    r = launch_case(case, device, arrays=a)
    assert (r.flags, r.prior_flags) == (0, nat.FLAG_SUPPORT)
    # a bad likelihood value is the site's alone
    a = dict(inputs(case))
    a["y"] = a["y"].copy()
    a["y"][N - 1] = np.nan
    r = launch_case(case, device, arrays=a)
    assert (r.flags, r.prior_flags) == (nat.FLAG_SUPPORT, 0)
    # MI_GROUP_FLAGS_ZEROED: the caller's zeroed words are ORed into, not cleared
    r = launch_case(case, device, arrays=a, flags_zeroed=True)
    assert (r.flags, r.prior_flags) == (nat.FLAG_SUPPORT, 0)


@pytest.mark.parametrize("case,valu", EXTREME,
                         ids=[c.id + ("-valu" if v else "-mfma") for c, v in EXTREME])
def test_extreme_regimes(device, case, valu):
    """
    Bernoulli logits of magnitude 20, 90 (exp(-|l|) denormal) and 200 (underflow) with y agreeing
    and disagreeing with their sign; Normal sigma of 1e-3 / 30 per particle and a constant 1e-2 with
    residuals of order 1. Values and gradients finite and within the bounds.
    """
    if case.regime.startswith("logit"):
        a = inputs(case)
        logits = np.abs(a["X"].astype(np.float64) @ a["theta"][:8].astype(np.float64).T)
        M = float(case.regime[5:])
        assert 0.5 * M < np.median(logits) < 2 * M
    compare(case, launch_case(case, device, valu))


@pytest.mark.parametrize("path", list(PATHS))
def test_flags_on_every_path(device, path):
    N, K, expect, valu = PATHS[path]
    case = Case(N_, N, 32, K, masked=True, per_particle=True, expect=expect)
    assert K % 32 != 0 and case.geometry(valu).last_stage_rows not in (0, 64, 128)
    clean = inputs(case)

    def flags_with(**changed):
        a = dict(clean)
        for name, (index, value) in changed.items():
            a[name] = a[name].copy()
            a[name][index] = value
        return launch_case(case, device, valu, arrays=a).flags

    assert flags_with() == 0
    # the last row of the ragged last stage
    assert flags_with(mask=(N - 1, True), y=(N - 1, np.nan)) == nat.FLAG_SUPPORT
    assert flags_with(mask=(N - 1, False), y=(N - 1, np.nan)) == 0
    # the last particle, in a particle tile that K does not fill
    assert flags_with(sigma=(K - 1, 0.0)) == nat.FLAG_PARAM
    assert flags_with(sigma=(K - 1, -1.0)) == nat.FLAG_PARAM
    assert flags_with(theta=((K - 1, 31), np.nan)) == nat.FLAG_PARAM
    assert flags_with(theta=((0, 0), np.nan), y=(N - 1, np.nan), mask=(N - 1, True)) == \
        (nat.FLAG_PARAM | nat.FLAG_SUPPORT)
    # Bernoulli: a value outside {0, 1}
    bern = Case(B_, N, 32, K, masked=True, expect=expect)
    a = dict(inputs(bern))
    a["y"], a["mask"] = a["y"].copy(), a["mask"].copy()
    a["y"][N - 1], a["mask"][N - 1] = 2.0, True
    assert launch_case(bern, device, valu, arrays=a).flags == nat.FLAG_SUPPORT
    a["mask"][N - 1] = False
    assert launch_case(bern, device, valu, arrays=a).flags == 0
