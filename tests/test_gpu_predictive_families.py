"""
Predictive draws of the discrete and heavy-tailed families on the HIP samplers
(csrc/predictive.hip): known answers against tests/predictive_reference.py at kernel level, and
the sites drawn inside ``broadcast_samples``.

Shapes: S in {1, 5, 33} x M in {1, 3, 4, 5, 257} (quad tails, a lone element, more than one
workgroup), each parameter as a per-sample scalar, a per-element constant and dense.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Beta, Binomial, Categorical, Normal

import mininf_amd as mi
from mininf_amd import _native as nat, predictive
from tests import example_models as ex, predictive_reference as ref

pytestmark = pytest.mark.gpu

CODES = {"bernoulli_probs": nat.PRED_BERNOULLI_PROBS, "bernoulli_logits": nat.PRED_BERNOULLI_LOGITS,
         "exponential": nat.PRED_EXPONENTIAL, "laplace": nat.PRED_LAPLACE,
         "cauchy": nat.PRED_CAUCHY, "half_cauchy": nat.PRED_HALF_CAUCHY,
         "half_normal": nat.PRED_HALF_NORMAL, "log_normal": nat.PRED_LOG_NORMAL}

# Relative tolerance against the float64 reference, per family: four times the largest error
# measured on the MI355X over every case below, and no looser than 1e-4. The error is measured as
# predictive_reference.relative_error states it. Measured maxima beside each bound.
RTOL = {
    "exponential": 9.2e-7,   # measured 2.293e-07
    "laplace": 3.9e-7,       # measured 9.817e-08
    "cauchy": 6.3e-7,        # measured 1.574e-07
    "half_cauchy": 7.3e-7,   # measured 1.824e-07
    "half_normal": 2.9e-6,   # measured 7.224e-07 (the hardware sine / cosine near their zeros)
    "log_normal": 6.5e-7,    # measured 1.613e-07
}
assert max(RTOL.values()) <= 1e-4
MARKED_CAP = 0.01


def _strided_device(array, S, M, device, transposed=False):
    """A [S, 1], [1, M] or [S, M] float32 array on the device and its (stride_s, stride_j)."""
    if transposed:
        held = torch.as_tensor(np.ascontiguousarray(array.T), device=device)
        return held, 1, S
    held = torch.as_tensor(np.ascontiguousarray(array), device=device)
    rows, cols = array.shape
    return held, (cols if rows > 1 else 0), (1 if cols > 1 else 0)


def launch_fixed(family, params, S, M, seed, stream_id, device, transposed=False):
    held = [_strided_device(p, S, M, device, transposed and p.shape == (S, M)) for p in params]
    out = torch.full((S * M,), float("nan"), dtype=torch.float32, device=device)
    (a, a_ss, a_sj), (b, b_ss, b_sj) = held[0], held[-1]
    nat.check(nat.lib().mi_predictive_sample(
        CODES[family], a.data_ptr(), a_ss, a_sj, b.data_ptr() if len(held) == 2 else None, b_ss,
        b_sj, S, M, seed, stream_id, out.data_ptr(), nat.stream_handle(device)), family)
    return out.cpu().numpy().astype(np.float64).reshape(S, M)


def philox_normals(S, M, seed, stream_id, device):
    eps = torch.empty(S * M, dtype=torch.float32, device=device)
    nat.check(nat.lib().mi_philox_normal(1, S * M, seed, 0, stream_id, 0, eps.data_ptr(),
                                         nat.stream_handle(device)), "mi_philox_normal")
    return eps.cpu().numpy().astype(np.float64).reshape(S, M)


@pytest.mark.parametrize("family", sorted(ref.FIXED))
def test_fixed_consumption_known_answers(device, family):
    worst, marks, draws, left_out = 0.0, 0, 0, 0
    for S, M in ref.SHAPES:
        for layout in ref.LAYOUTS:
            params = ref.fixed_parameters(family, S, M, layout)
            want, marked, u = ref.fixed_draw(family, params, ref.SEED, ref.FIXED_STREAM, S, M)
            got = launch_fixed(family, params, S, M, ref.SEED, ref.FIXED_STREAM, device)
            assert np.isfinite(got).all(), (S, M, layout)
            draws += S * M
            if layout == "dense":   # the same parameter stored transposed: strides (1, S)
                again = launch_fixed(family, params, S, M, ref.SEED, ref.FIXED_STREAM, device, transposed=True)
                assert np.array_equal(got, again), (S, M)
            if family == "bernoulli_probs":
                assert np.array_equal(got, want), (S, M, layout)
                continue
            if family == "bernoulli_logits":
                marks += int(marked.sum())
                assert np.array_equal(got[~marked], want[~marked]), (S, M, layout)
                continue
            keep = ref.tangent_compared(u) if "cauchy" in family else np.ones((S, M), bool)
            left_out += int((~keep).sum())
            full = [np.broadcast_to(p, (S, M)) for p in params]
            error = ref.relative_error(family, [p[keep] for p in full], got[keep], want[keep])
            worst = max(worst, float(error.max()))
            if family in ("half_normal", "log_normal"):
                # the draw is that function of the generator's own normal for the element
                eps = philox_normals(S, M, ref.SEED, ref.FIXED_STREAM, device)
                exact = full[0] * np.abs(eps) if family == "half_normal" else \
                    np.exp(full[0] + eps * full[1])
                np.testing.assert_allclose(got, exact, rtol=2e-7, atol=0)
    print(f"{family}: largest relative error {worst:.3e} over {draws} draws, "
          f"{left_out} left out, {marks} marked")
    assert marks <= MARKED_CAP * draws
    assert left_out <= 0.002 * draws
    if family in RTOL:
        assert worst <= RTOL[family], worst


def launch_categorical(logits, strides, S, T, B, C, seed, stream_id, device):
    held = torch.as_tensor(logits, device=device)
    out = torch.full((S * T * B,), -1, dtype=torch.int64, device=device)
    nat.check(nat.lib().mi_predictive_categorical(
        held.data_ptr(), *strides, S, T, B, C, seed, stream_id, out.data_ptr(),
        nat.stream_handle(device)), "mi_predictive_categorical")
    return out.cpu().numpy()


def test_categorical_known_answers(device):
    marks = draws = 0
    S = ref.CATEGORICAL_S
    for C, B, T in ref.CATEGORICAL_CASES:
        for layout in ("dense", "element"):
            logits = ref.categorical_logits(C, B, layout)
            shared = np.broadcast_to(logits, (S, B, C))
            rows = ref.categorical_rows(shared, T)
            u = ref.uniforms(ref.SEED, 11, len(rows))
            want, marked = ref.categorical(rows, u)
            strides = (B * C if layout == "dense" else 0, C, 1)
            got = launch_categorical(logits, strides, S, T, B, C, ref.SEED, 11, device)
            assert got.min() >= 0 and got.max() < C, (C, B, T, layout)
            assert np.array_equal(got[~marked], want[~marked]), (C, B, T, layout)
            # never a category of zero weight
            assert np.isfinite(rows[np.arange(len(rows)), got]).all(), (C, B, T, layout)
            marks, draws = marks + int(marked.sum()), draws + len(rows)
    print(f"categorical: {marks} of {draws} draws marked")
    assert marks <= MARKED_CAP * draws


def test_categorical_frequencies(device):
    """20000 rows of one distribution: each frequency within 5 standard errors of softmax."""
    for C in (5, 40):   # one thread per row / one wave per row
        logits = np.linspace(-2.0, 1.0, C).astype(np.float32).reshape(1, 1, C)
        R = 20000
        got = launch_categorical(logits, (0, 0, 1), R, 1, 1, C, ref.SEED, 12, device)
        p = np.exp(logits.reshape(-1).astype(np.float64))
        p /= p.sum()
        freq = np.bincount(got, minlength=C) / R
        assert (np.abs(freq - p) < 5 * np.sqrt(p * (1 - p) / R)).all(), (C, freq, p)


@pytest.fixture(scope="module")
def poisson_draws(device):
    S, M = ref.POISSON_SHAPE
    rates = ref.poisson_rates()
    held = torch.as_tensor(rates, device=device)
    out = torch.full((S * M,), -1.0, dtype=torch.float32, device=device)
    nat.check(nat.lib().mi_predictive_poisson(held.data_ptr(), M, 1, S, M, ref.SEED, 9,
                                              out.data_ptr(), nat.stream_handle(device)),
              "mi_predictive_poisson")
    return rates.reshape(-1), out.cpu().numpy().astype(np.float64)


def test_poisson_known_answers(poisson_draws):
    rates, got = poisson_draws
    want, marked, _ = ref.poisson(rates, ref.SEED, 9)
    print(f"poisson: {int(marked.sum())} of {len(got)} draws marked")
    assert marked.mean() <= MARKED_CAP
    assert np.array_equal(got[~marked], want[~marked])
    assert (got[rates == 0] == 0).all()


def test_poisson_moments(poisson_draws):
    rates, got = poisson_draws
    for rate in (3.0, 37.5):
        x, n = got[rates == np.float32(rate)], int((rates == np.float32(rate)).sum())
        assert abs(x.mean() - rate) < 5 * np.sqrt(rate / n), rate
        assert abs(x.var(ddof=1) - rate) < 5 * np.sqrt((rate + 2.0 * rate * rate) / n), rate


def test_poisson_strides_and_invalid_rates(device):
    """A per-sample scalar and a per-element constant read in place give what the dense
    parameter gives; a negative or non-finite rate writes NaN."""
    S, M = 5, 257
    lib, stream = nat.lib(), nat.stream_handle(device)
    per_sample = torch.tensor([0.5, 4.0, 9.0, 12.0, 300.0], device=device)
    per_element = torch.linspace(0.1, 60.0, M, device=device)
    for held, ss, sj in ((per_sample, 1, 0), (per_element, 0, 1)):
        dense = (held[:, None] if ss else held[None, :]).expand(S, M).contiguous()
        outs = []
        for t, a, b in ((held, ss, sj), (dense, M, 1)):
            out = torch.empty(S * M, dtype=torch.float32, device=device)
            nat.check(lib.mi_predictive_poisson(t.data_ptr(), a, b, S, M, ref.SEED, 9,
                                                out.data_ptr(), stream), "mi_predictive_poisson")
            outs.append(out)
        assert torch.equal(*outs)
        want, marked, _ = ref.poisson(dense.cpu().numpy(), ref.SEED, 9)
        got = outs[0].cpu().numpy().astype(np.float64)
        assert np.array_equal(got[~marked], want[~marked])
    bad = torch.tensor([-1.0, float("nan"), float("inf"), 2.0], device=device)
    out = torch.empty(4, dtype=torch.float32, device=device)
    nat.check(lib.mi_predictive_poisson(bad.data_ptr(), 0, 1, 1, 4, ref.SEED, 9, out.data_ptr(),
                                        stream), "mi_predictive_poisson")
    assert torch.isnan(out[:3]).all() and float(out[3]) >= 0


def test_invalid_sizes_launch_nothing(device):
    lib, stream = nat.lib(), nat.stream_handle(device)
    p = torch.zeros(4, device=device)
    o = torch.zeros(4, dtype=torch.int64, device=device)
    assert lib.mi_predictive_categorical(p.data_ptr(), 0, 0, 1, 1, 1, 1, 0, 0, 0, o.data_ptr(),
                                         stream) == nat.MI_EINVAL
    assert lib.mi_predictive_categorical(p.data_ptr(), 0, 0, 1, 1, 1, 1, 1025, 0, 0, o.data_ptr(),
                                         stream) == nat.MI_EUNSUPPORTED
    assert lib.mi_predictive_sample(0, p.data_ptr(), 0, 0, None, 0, 0, 1 << 20, (1 << 14) + 1, 0, 0,
                                    p.data_ptr(), stream) == nat.MI_EUNSUPPORTED
    assert lib.mi_predictive_poisson(p.data_ptr(), 0, 0, 1 << 20, (1 << 12) + 1, 0, 0,
                                     p.data_ptr(), stream) == nat.MI_EUNSUPPORTED
    torch.cuda.synchronize()
    assert float(p.abs().sum()) == 0 and int(o.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------
# Through broadcast_samples
# ------------------------------------------------------------------------------------------------
S_COIN, N_COIN = 33, 257


def coin():
    theta = mi.sample("theta", Beta(2, 2))
    mi.sample("x", Bernoulli(theta), sample_shape=[N_COIN])


def _seed_of(manual_seed):
    torch.manual_seed(manual_seed)
    return int(torch.randint(0, 2 ** 62, ()).item())


@pytest.fixture(scope="module")
def coin_run(device):
    torch.manual_seed(11)
    theta = Beta(2.0, 2.0).sample([S_COIN]).to(device)
    predictive.reset_counts()
    torch.manual_seed(3)
    out = mi.broadcast_samples(coin, mi.State({"theta": theta}))
    return theta, out, predictive.native_draws()


def test_readme_model_draws_bernoulli_natively(coin_run):
    theta, out, counts = coin_run
    assert counts["Bernoulli"] == 1 and sum(counts.values()) == 1
    x = out["x"]
    assert x.shape == (S_COIN, N_COIN) and x.dtype == torch.float32 and x.is_cuda
    u = ref.uniforms(_seed_of(3), predictive.STREAM_BASE + 0, S_COIN * N_COIN)
    want = ref.bernoulli_probs(theta.cpu().numpy()[:, None], u.reshape(S_COIN, N_COIN))
    assert np.array_equal(x.cpu().numpy(), want)


def test_shards_reproduce_the_prefix(coin_run):
    """A draw depends on (seed, stream, s, j, M) with s counted within the call. So samples
    0-16 broadcast alone are rows 0-16 of the full run bit for bit (the prefix property), while a
    shard that starts at sample 17 numbers its samples from 0: its rows are the reference's draws
    for its own s, not rows 17-32 of the full run (there is no sample offset to pass)."""
    theta, full, _ = coin_run
    torch.manual_seed(3)
    head = mi.broadcast_samples(coin, mi.State({"theta": theta[:17]}))
    assert torch.equal(head["x"], full["x"][:17])
    torch.manual_seed(3)
    tail = mi.broadcast_samples(coin, mi.State({"theta": theta[17:]}))
    u = ref.uniforms(_seed_of(3), predictive.STREAM_BASE + 0, S_COIN * N_COIN)[:16 * N_COIN]
    want = ref.bernoulli_probs(theta[17:].cpu().numpy()[:, None], u.reshape(16, N_COIN))
    assert np.array_equal(tail["x"].cpu().numpy(), want)


def test_poisson_and_categorical_sites(device):
    S = 8
    torch.manual_seed(5)
    states = mi.State({
        "population_scale": torch.rand(S, device=device) + 0.5,
        "z": torch.randn(S, ex.FEATURE_N, device=device),
        "noise_scale": torch.rand(S, device=device) + 0.5,
        "intercept": torch.randn(S, device=device),
        "slope": 0.5 * torch.randn(S, device=device)})
    predictive.reset_counts()
    out = mi.broadcast_samples(ex.feature_model, states)
    assert predictive.native_draws() == {"Normal": 1, "Poisson": 1}
    y = out["y"]
    assert y.shape == (S, ex.FEATURE_N) and y.dtype == torch.float32 and y.is_cuda
    assert bool(((y >= 0) & (y == y.round())).all())
    rate = (states["intercept"][:, None] + states["z"] * states["slope"][:, None]).exp()
    assert _counts_near(y, rate)

    def model():
        w = mi.sample("w", Normal(0, 1), sample_shape=[3])
        mi.sample("c", Categorical(logits=w), sample_shape=[5])

    w = torch.randn(S, 3, device=device)
    predictive.reset_counts()
    c = mi.broadcast_samples(model, mi.State({"w": w}))["c"]
    assert predictive.native_draws() == {"Categorical": 1}
    like = Categorical(logits=w[0]).sample([5])
    assert c.shape == (S,) + like.shape and c.dtype == like.dtype == torch.int64 and c.is_cuda
    assert int(c.min()) >= 0 and int(c.max()) < 3


def _counts_near(y, rate):
    """Every count within 8 standard deviations (+ 8) of its rate."""
    return bool(((y - rate).abs() <= 8 * rate.sqrt() + 8).all())


def test_binomial_site_keeps_torch(device):
    def model():
        theta = mi.sample("theta", Beta(2, 2))
        mi.sample("k", Binomial(10, probs=theta), sample_shape=[4])

    theta = torch.rand(6, device=device) * 0.8 + 0.1
    predictive.reset_counts()
    k = mi.broadcast_samples(model, mi.State({"theta": theta}))["k"]
    assert k.shape == (6, 4) and bool(((k >= 0) & (k <= 10)).all())
    assert sum(predictive.native_draws().values()) == 0
