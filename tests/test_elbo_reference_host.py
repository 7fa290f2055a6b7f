"""
The float64 yardstick of the ELBO tail (tests/elbo_reference.py) checked without a GPU:
  - against torch.distributions' entropies and float64 autograd, so it does not share the
    kernels' formulae;
  - the form of the error bound, on a float32 restatement of csrc/entropy.hpp's digammaf /
    trigammaf and csrc/elbo.hip's entropy expressions;
  - the launch-plan branch every designed shape of tests/test_gpu_elbo_tail.py is meant for, on a
    restatement of make_layout / add_absorbed (csrc/elbo.hip).
"""
import math

import numpy as np
import pytest
import torch
from scipy import special

from tests import elbo_reference as ref

f32 = np.float32
C = 4.0   # error <= C * 2^-24 * magnitude


# ---- the reference against torch.distributions -------------------------------------------------

def _torch_entropy(dist, params, exp):
    """entropy() and its float64 gradients: through exp of an unconstrained leaf when exp."""
    leaves = [torch.tensor(np.log(p) if exp else p, dtype=torch.float64, requires_grad=True)
              for p in params]
    h = dist(*[leaf.exp() if exp else leaf for leaf in leaves]).entropy()
    h.sum().backward()
    return h.detach().numpy(), np.stack([leaf.grad.numpy() for leaf in leaves], -1)


TORCH_TRIGAMMA = 1e-9   # torch's float64 polygamma(1, .) against mpmath: 4.8e-10 relative at 1


def _close(got, want, what, trigamma=None):
    """1e-12 relative; a gradient torch forms with its float64 trigamma also gets that function's
    own error, relative to the trigamma terms' magnitude."""
    err = np.abs(np.asarray(got) - want)
    tol = 1e-12 * np.maximum(np.abs(want), 1e-300)
    if trigamma is not None:
        tol = tol + TORCH_TRIGAMMA * trigamma
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:5], float((err / tol).max()))


@pytest.mark.parametrize("exp", [False, True])
def test_reference_matches_torch_entropies(exp):
    conc = np.asarray(ref.CONCENTRATIONS, np.float64)
    rates = np.asarray(ref.RATES, np.float64)
    # Normal: every scale of the rate set (the loc has no part in the entropy)
    h, _, d, _ = ref.normal_entropy(rates)
    th, tg = _torch_entropy(lambda s: torch.distributions.Normal(torch.zeros_like(s), s), [rates],
                            exp)
    _close(h, th, "normal entropy")
    _close(d[:, 1] * (rates if exp else 1.0), tg[:, 0], "normal gradient")
    # Gamma: every concentration with every rate
    a, r = (v.ravel() for v in np.meshgrid(conc, rates))
    h, _, d, dmag = ref.gamma_entropy(a, r)
    th, tg = _torch_entropy(torch.distributions.Gamma, [a, r], exp)
    chain = np.stack([a, r], -1) if exp else 1.0
    # (a + lgamma(a) + (1 - a) psi(a) cancels at 1e4, and exp(log(a)) is not a: relative to the
    # summands)
    assert (np.abs(h - th) <= 1e-12 * np.maximum(np.abs(th), ref.gamma_entropy(a, r)[1])).all()
    _close(d * chain, tg, "gamma gradient", trigamma=dmag * chain)
    # Beta: the designed pairs, both ways round, with the exact total torch forms in float64
    pairs = np.asarray(ref.BETA_PAIRS + tuple((b, a) for a, b in ref.BETA_PAIRS), np.float64)
    a, b = pairs[:, 0], pairs[:, 1]
    h, _, d, _ = ref.beta_entropy(a, b, a + b)
    th, tg = _torch_entropy(torch.distributions.Beta, [a, b], exp)
    # (torch's own float64 lgamma / digamma cancel at (1e4, 1e4): relative to the summands there)
    tol = 1e-12 * np.maximum(np.abs(th), ref.beta_entropy(a, b, a + b)[1])
    assert (np.abs(h - th) <= tol).all(), (h, th)
    chain = np.stack([a, b], -1) if exp else 1.0
    _close(d * chain, tg, "beta gradient", trigamma=ref.beta_entropy(a, b, a + b)[3] * chain)


def test_reference_derivatives_match_mpmath():
    """The reference's digamma / trigamma terms to 1e-12 against 40-digit arithmetic: torch's
    float64 trigamma (the autograd check above) is itself only good to 5e-10."""
    import mpmath
    with mpmath.workdps(40):
        psi1 = lambda v: mpmath.polygamma(1, mpmath.mpf(float(v)))   # noqa: E731
        for a in ref.CONCENTRATIONS:
            _, _, d, _ = ref.gamma_entropy(a, 1.0)
            want = float(1 + (1 - mpmath.mpf(a)) * psi1(a))
            assert abs(d[0] - want) <= 1e-12 * max(abs(want), 1 + abs(1 - a) * float(psi1(a)))
            assert abs(float(special.polygamma(1, a)) - float(psi1(a))) <= 1e-12 * float(psi1(a))
        for a, b in ref.BETA_PAIRS:
            _, _, d, dmag = ref.beta_entropy(a, b, a + b)
            t = mpmath.mpf(a) + mpmath.mpf(b)
            for j, p in enumerate((a, b)):
                want = float((t - 2) * psi1(t) - (mpmath.mpf(p) - 1) * psi1(p))
                assert abs(d[j] - want) <= 1e-12 * max(abs(want), dmag[j]), (a, b, j)


def test_reference_elbo_composes_entropies_terms_and_chain_rule():
    """The whole reference on a small case against torch autograd of the same loss in float64."""
    rng = np.random.default_rng(0)
    K, n = 5, 4
    terms = [rng.normal(size=K).astype(f32) for _ in range(2)]
    src = [rng.normal(size=(K, n)).astype(f32) for _ in range(2)]
    eps = rng.normal(size=(K, n)).astype(f32)
    loc, scale = rng.normal(size=n).astype(f32), rng.uniform(0.5, 2, n).astype(f32)
    a, r = rng.uniform(0.5, 3, n).astype(f32), rng.uniform(0.5, 3, n).astype(f32)
    case = {"K": K, "g0": f32(-1.0 / K), "entropy_scale": 0.5, "terms": terms, "factors": [
        {"family": "normal", "n": n, "p0": loc, "p1": scale, "weight": 0.25, "transform": (0, 1),
         "draw": "sources", "sources": src, "eps": eps},
        {"family": "gamma", "n": n, "p0": a, "p1": r, "weight": 1.0, "transform": (1, 0),
         "draw": None}]}
    u = f32(2.5)
    out = ref.elbo_reference(case, u)
    g0 = float(f32(-1.0 / K))
    dz = torch.tensor(ref.source_sum(src, (K, n)).astype(np.float64))
    t = lambda v, g=True: torch.tensor(np.asarray(v, np.float64), requires_grad=g)   # noqa: E731
    tl, tus, tua, tr = t(loc), t(np.log(scale.astype(np.float64))), t(np.log(a.astype(np.float64))), t(r)
    z = tl + t(eps, False) * tus.exp()
    h = 0.25 * torch.distributions.Normal(tl, tus.exp()).entropy().sum() + \
        torch.distributions.Gamma(tua.exp(), tr).entropy().sum()
    loss = g0 * sum(float(np.asarray(x, np.float64).sum()) for x in terms) - 0.5 * h
    # the draws' backward: the sources are d(g0 T)/dz, so their part of the loss is <dz, z>
    (float(u) * (loss + (dz * z).sum())).backward()
    loss = float(loss.detach())
    assert abs(float(out["loss"].value) - loss) <= 1e-12 * abs(loss)
    _close(out["grads"][0].value, np.stack([tl.grad.numpy(), tus.grad.numpy()], -1), "normal")
    _close(out["grads"][1].value, np.stack([tua.grad.numpy(), tr.grad.numpy()], -1), "gamma",
           trigamma=out["grads"][1].mag["gamma"])
    assert float(out["dterm"].value) == float(u) * g0


def test_reference_reductions_on_a_hand_case():
    K = 3
    job = {"nseg": 2, "num_sites": 2, "num_slots": 1, "scale": [2.0, -0.5], "slot_scale": 3.0,
           "values": [np.asarray([[1, 2, 3], [4, 5, 6]], f32),
                      {"u": np.asarray([1, 2], f32), "f": np.asarray([1, 0, -1], f32),
                       "e": np.asarray([10, 20, 30], f32)},
                      np.asarray([[1, 1, 1], [0.5, 0.5, 0.5]], f32)], "ksum": None}
    r = ref.reduce_job(job, K)
    assert np.array_equal(r["site_lp"].value, [[10, 14, 18], [-6.5, -10, -13.5]])
    assert np.array_equal(r["total"].value, [3.5, 4, 4.5])
    assert np.array_equal(r["slot_grad"].value, [[4.5, 4.5, 4.5]])
    ks = dict(job, num_sites=1, scale=[2.0], values=job["values"][2:],
              ksum=np.asarray([[1.0, 2.0, 4.0]]))
    case = {"K": K, "g0": f32(-0.5), "entropy_scale": 1.0, "jobs": [job, ks]}
    out = ref.elbo_reference(case)
    assert float(out["loss"].value) == -0.5 * (12.0 + 2.0 * 7.0)
    assert out["jobs"][1]["total"] is None


# ---- the form of the bound, on a float32 restatement of the device expressions -----------------

def digammaf(x):
    """csrc/entropy.hpp's digammaf, step by step in float32."""
    x = f32(x)
    shift = f32(0)
    while x < f32(6):
        shift = f32(shift - f32(1) / x)
        x = f32(x + f32(1))
    r = f32(f32(1) / f32(x * x))
    inner = f32(f32(1) / f32(252) - f32(r * f32(f32(1) / f32(240))))
    inner = f32(f32(1) / f32(120) - f32(r * inner))
    series = f32(r * f32(f32(1) / f32(12) - f32(r * inner)))
    return f32(f32(f32(shift + f32(np.log(x))) - f32(f32(0.5) / x)) - series)


def trigammaf(x):
    """csrc/entropy.hpp's trigammaf, step by step in float32."""
    x = f32(x)
    acc = f32(0)
    while x < f32(6):
        acc = f32(acc + f32(1) / f32(x * x))
        x = f32(x + f32(1))
    r = f32(f32(1) / f32(x * x))
    inner = f32(f32(1) / f32(42) - f32(r * f32(f32(1) / f32(30))))
    inner = f32(f32(1) / f32(30) - f32(r * inner))
    tail = f32(f32(r / x) * f32(f32(1) / f32(6) - f32(r * inner)))
    return f32(f32(f32(acc + f32(1) / x) + f32(f32(0.5) * r)) + tail)


def lgammaf(x):
    """An ideal lgammaf: the float64 value rounded once."""
    return f32(special.gammaln(float(f32(x))))


def _set():
    return [float(f32(v)) for v in ref.CONCENTRATIONS]


def test_float32_digamma_and_trigamma_fit_the_bound():
    worst = {"digamma": 0.0, "trigamma": 0.0}
    for a in _set():
        d = abs(float(digammaf(a)) - special.digamma(a)) / (ref.EPS32 * ref.digamma_magnitude(a))
        t = abs(float(trigammaf(a)) - special.polygamma(1, a)) / \
            (ref.EPS32 * special.polygamma(1, a))
        worst = {"digamma": max(worst["digamma"], float(d)), "trigamma": max(worst["trigamma"], float(t))}
    print("float32 restatement, worst error / (2^-24 magnitude):", worst)
    assert worst["digamma"] <= C and worst["trigamma"] <= C, worst


def test_float32_entropies_and_derivatives_fit_the_bound():
    """factor_entropy / entropy_grad_of of csrc/elbo.hip in float32 against scipy, on the
    concentration set with every rate (Gamma) and the designed pairs (Beta)."""
    one, two = f32(1), f32(2)
    worst = {}

    def note(key, got, want, mag):
        if mag == 0.0:
            assert got == want, (key, got, want)
            return
        worst[key] = max(worst.get(key, 0.0), abs(float(got) - float(want)) / (ref.EPS32 * float(mag)))

    for s in ref.RATES:
        s = f32(s)
        h, mag, d, dmag = ref.normal_entropy(float(s))
        note("normal value", float(f32(1.4189385332046727) + f32(np.log(s))), h,
             mag + 1.4189385332046727)   # (the element form rounds the constant too)
        note("normal gradient", one / s, d[1], dmag[1])
    for a in _set():
        a = f32(a)
        for r in ref.RATES:
            r = f32(r)
            h, mag, d, dmag = ref.gamma_entropy(float(a), float(r))
            got = float(f32(a - f32(np.log(r)))) + float(lgammaf(a)) + \
                float(f32(f32(one - a) * digammaf(a)))
            note("gamma value", got, h, mag)
            note("gamma gradient 0", f32(one + f32(f32(one - a) * trigammaf(a))), d[0], dmag[0])
            note("gamma gradient 1", f32(-one / r), d[1], dmag[1])
    for a, b in ref.BETA_PAIRS:
        a, b = f32(a), f32(b)
        t = f32(a + b)
        h, mag, d, dmag = ref.beta_entropy(float(a), float(b))
        got = float(f32(f32(lgammaf(a) + lgammaf(b)) - lgammaf(t))) - \
            float(f32(f32(two - t) * digammaf(t))) - float(f32(f32(a - one) * digammaf(a))) - \
            float(f32(f32(b - one) * digammaf(b)))
        note("beta value", got, h, mag)
        tt = f32(f32(t - two) * trigammaf(t))
        note("beta gradient 0", f32(tt - f32(f32(a - one) * trigammaf(a))), d[0], dmag[0])
        note("beta gradient 1", f32(tt - f32(f32(b - one) * trigammaf(b))), d[1], dmag[1])
    print("float32 restatement, worst error / (2^-24 magnitude):", worst)
    assert max(worst.values()) <= C, worst


def test_digamma_magnitude_counts_the_recurrence():
    assert ref.digamma_magnitude(6.0) == pytest.approx(math.log(6.0))
    assert ref.digamma_magnitude(5.999) == pytest.approx(1 / 5.999 + math.log(6.999))
    assert ref.digamma_magnitude(1.0) == pytest.approx(sum(1 / j for j in range(1, 6)) + math.log(6.0))
    # honest at psi's root, where |psi| itself is 0
    assert ref.digamma_magnitude(1.4616321) > 1.0 > 1e6 * abs(special.digamma(1.4616321))


# ---- the plan branches of the designed shapes ---------------------------------------------------

THREADS = 256


def ceil_div(a, b):
    return -(-a // b)


def lead_blocks(K, longest):
    """make_layout: about kLead = 32 elements per lane of the longest term or factor."""
    return max(1, min(1024, ceil_div(max(K, longest), 32 * THREADS)))


def absorbed(n, rows, per_lane, partials=False, quad=False):
    """add_absorbed: (tk, ti, columns, slices, epl). per_lane: 4, or for a forward-absorbed Beta
    16 with precomputed factors and 1 without."""
    tk = 1
    while tk < THREADS and tk < ceil_div(rows, per_lane):
        tk <<= 1
    ti = THREADS // tk
    need = 1
    while need < ti and need < n:
        need <<= 1
    if need < ti:
        ti, tk = need, THREADS // need
    gx = ceil_div(n, ti)
    slices = max(1, min(ceil_div(rows, tk * per_lane), ceil_div(2048, gx)))
    slices = ceil_div(rows, ceil_div(rows, slices))
    epl = 4 if partials and tk == 1 and slices == 1 else 1
    if epl == 4 and quad:
        epl = -2
    return tk, ti, gx, slices, epl


def kred(nseg, K):
    if nseg >= 768 and K < 2048:
        return 8
    if nseg >= 512 and K < 2048:
        return 16
    return 32 if nseg >= 64 else 64


def test_designed_shapes_land_in_their_plan_branches():
    for n, blocks in ref.NORMAL_N.items():
        for K in (1, 3, 256):
            assert lead_blocks(K, n) == blocks, (n, K)
    assert lead_blocks(8193, 5) == 2
    # 8191 in one lead block: lanes 0..254 take the 8-quad round, lane 255 the 4-quad round and
    # then single quads; 3 elements are left to the scalar loop
    nq, stride = 8191 >> 2, THREADS
    assert 254 + 7 * stride < nq <= 255 + 7 * stride and 255 + 3 * stride < nq
    assert 255 + 4 * stride + 3 * stride >= nq > 255 + 4 * stride and 8191 - (nq << 2) == 3
    for (n, K), (tk, ti, gx, slices) in ref.NORMAL_SOURCES.items():
        assert absorbed(n, K, 4) == (tk, ti, gx, slices, 1), (n, K)
    assert ref.NORMAL_SOURCES[(5, 3)][0] > 3           # more row lanes than rows
    for (rows, n, gs), (tk, ti, epl) in ref.PARTIALS.items():
        quad = n % 4 == 0 and gs == 1
        assert absorbed(n, rows, 4, partials=True, quad=quad)[::4] == (tk, epl), (rows, n, gs)
        assert absorbed(n, rows, 4, partials=True, quad=quad)[1] == ti
    for (n, K), (tk, ti, slices) in ref.BETA_DGRAD.items():
        assert absorbed(n, K, 16)[:2] + absorbed(n, K, 16)[3:4] == (tk, ti, slices), (n, K)
    assert ref.BETA_DGRAD[(1, 17)][0] > 17             # the tree over tk lanes with K < tk
    for (nseg, K), want in ref.REDUCE.items():
        assert kred(nseg, K) == want, (nseg, K)
    assert sorted(set(ref.REDUCE.values())) == [8, 16, 32, 64]
