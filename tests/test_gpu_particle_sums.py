"""
Particle-summed site values (MI_GROUP_KSUM, mi_reduce.ksum): the Bernoulli BCAST kernel leaves one
fp64 sum per workgroup instead of a [chunks + 1, K] fp32 slab, and the ELBO forward adds those
doubles straight into the loss, in its reducing blocks -- or in its lead blocks when the launch is
too large to reduce its jobs itself and runs them as launches of their own first
(MININF_AMD_ELBO_EXTERNAL=1 takes that path at any size).

Reference for every comparison: the same step with MININF_AMD_BCAST_KSUM=0 (the per-particle form)
and, for the Beta-Bernoulli model, the fp64 oracle on the restated draws at 1e-5 (the bound of the
existing C2 tests). The loss differs from the per-particle form only by the association of an fp64
sum and one fp32 rounding per particle less: rel 1e-6, as test_gpu_fused_reduce.py.
"""
import ctypes

import pytest
import torch
from torch.distributions import Bernoulli, Beta, Normal

import mininf_amd as mi
from mininf_amd import _native as nat
from mininf_amd import engine
from mininf_amd.particles import SiteRecord
from mininf_amd.graph import StepGraph
from mininf_amd.optim import Adam
from oracle import build as oracle_build
from oracle import elbo as oracle

pytestmark = pytest.mark.gpu

SEED = 11
C1, C0 = 1.5, 2.5
# K: one partial particle block / a partial second block (lanes past K) / five blocks, the last
# nearly empty. n: 2 chunks (chunk 0 takes every constant
# slot) / >= 4 chunks (spread constants) / an odd tail element / a chunk count padded to 8.
KS = [512, 1500, 4100]
NS = [5000, 20000, 12321, 4096 * 9 + 33]


def data(n):
    gen = torch.Generator().manual_seed(3)
    return (torch.rand(n, generator=gen) < 0.3).float()


def coin(device, x, form):
    n = x.numel()
    if form == "probs":
        def model():
            theta = mi.sample("theta", Beta(2, 2))
            mi.sample("x", Bernoulli(theta), sample_shape=[n])
        module = mi.nn.ParameterizedDistribution(Beta, concentration1=C1,
                                                 concentration0=C0).to(device)
    else:
        def model():
            z = mi.sample("theta", Normal(0.0, 1.0))
            mi.sample("x", Bernoulli(logits=z), sample_shape=[n])
        module = mi.nn.ParameterizedDistribution(Normal, loc=-0.4, scale=0.3).to(device)
    return mi.condition(model, x=x.to(device)), module


def evaluate(device, monkeypatch, x, K, form, ksum, steps=2, env=()):
    monkeypatch.setenv("MININF_AMD_BCAST_KSUM", "1" if ksum else "0")
    for name, value in env:
        monkeypatch.setenv(name, value)
    conditioned, module = coin(device, x, form)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=SEED)
    out = []
    for _ in range(steps):
        module.zero_grad()
        loss = loss_fn(conditioned, {"theta": module()})
        loss.backward()
        grads = {name: p.grad.clone() for name, p in module.distribution_parameters.items()}
        out.append((loss.detach().clone(), grads, dict(loss_fn.last_fusions)))
    for name, _ in env:
        monkeypatch.delenv(name)
    return out


def check_against(on, off):
    for (lo, go, _), (lf, gf, _) in zip(on, off):
        print("loss", float(lo), float(lf), {k: (float(go[k]), float(gf[k])) for k in go})
        assert float(lo) == pytest.approx(float(lf), rel=1e-6)
        for name in go:
            torch.testing.assert_close(go[name], gf[name], rtol=1e-5, atol=1e-6)


def check_oracle(x, K, on):
    xs = x.numpy()
    for step, (loss, grads, _) in enumerate(on):
        # (the parameters do not move: no optimizer step between the evaluations)
        draws = oracle_build.beta_draws([C1], [C0], K, SEED, step, 0, 0)[0][:, 0]
        ref = oracle.beta_bernoulli_elbo(xs, 2, 2, C1, C0, draws)
        print("oracle", step, float(loss), ref["loss"])
        assert abs(float(loss) - ref["loss"]) <= 1e-5 * abs(ref["loss"]), step
        for name in ("concentration1", "concentration0"):
            want = ref[f"grad_u_{name}"]
            assert abs(float(grads[name]) - want) <= 1e-5 * abs(want), (step, name)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_probs_against_the_per_particle_form_and_the_oracle(device, monkeypatch, K, n):
    x = data(n)
    on = evaluate(device, monkeypatch, x, K, "probs", True)
    off = evaluate(device, monkeypatch, x, K, "probs", False)
    for _, _, fusions in on:
        assert fusions["particle_sums"] == 1 and fusions["deferred_reductions"] == 1
        assert fusions["final_grads"] == 1
    for _, _, fusions in off:
        assert fusions["particle_sums"] == 0
    check_against(on, off)
    check_oracle(x, K, on)


@pytest.mark.parametrize("form,K,n", [("probs", 1500, 20000), ("probs", 4100, 12321),
                                      ("probs", 512, 5000), ("logits", 1500, 20000)])
def test_a_launch_that_reduces_its_jobs_on_their_own(device, monkeypatch, form, K, n):
    """An ELBO launch too large for its completion counters runs its reductions as launches of
    their own first (here forced at a small size): of a particle-summed job only the slots, and
    the lead blocks add the doubles. Such a launch leaves the final gradients to the backward,
    which is how the test sees that the path was taken."""
    x = data(n)
    on = evaluate(device, monkeypatch, x, K, form, True,
                  env=[("MININF_AMD_ELBO_EXTERNAL", "1")])
    off = evaluate(device, monkeypatch, x, K, form, False)
    for _, _, fusions in on:
        assert fusions["particle_sums"] == 1 and fusions["deferred_reductions"] == 1
        assert fusions["final_grads"] == 0
    for _, _, fusions in off:
        assert fusions["particle_sums"] == 0
    check_against(on, off)
    if form == "probs":
        check_oracle(x, K, on)


@pytest.mark.parametrize("n", [5000, 20000])
def test_closed_form_measurement_path(device, monkeypatch, n):
    """MININF_AMD_BCAST_SUFFSTAT=1 (the floor measurement) goes through the same epilogue."""
    x = data(n)
    suff = [("MININF_AMD_BCAST_SUFFSTAT", "1")]
    on = evaluate(device, monkeypatch, x, 1500, "probs", True, env=suff)
    off = evaluate(device, monkeypatch, x, 1500, "probs", False, env=suff)
    for _, _, fusions in on:
        assert fusions["particle_sums"] == 1
    check_against(on, off)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_logits_against_the_per_particle_form(device, monkeypatch, K, n):
    """(oracle.elbo restates no logits model: the per-particle form is the reference)"""
    x = data(n)
    on = evaluate(device, monkeypatch, x, K, "logits", True)
    off = evaluate(device, monkeypatch, x, K, "logits", False)
    for _, _, fusions in on:
        assert fusions["particle_sums"] == 1
    for _, _, fusions in off:
        assert fusions["particle_sums"] == 0
    check_against(on, off)


@pytest.mark.parametrize("K", [1500, 4100])
def test_same_seed_and_step_give_the_same_bits(device, monkeypatch, K):
    x = data(20000)
    a = evaluate(device, monkeypatch, x, K, "probs", True)
    b = evaluate(device, monkeypatch, x, K, "probs", True)
    for (la, ga, fa), (lb, gb, _) in zip(a, b):
        assert fa["particle_sums"] == 1
        assert torch.equal(la, lb)
        for name in ga:
            assert torch.equal(ga[name], gb[name])


def train(device, monkeypatch, held, steps, graph=False, K=1024, n=20000):
    monkeypatch.setenv("MININF_AMD_BCAST_KSUM", "1")
    monkeypatch.setenv("MININF_AMD_DEFER_STEP", "1" if held else "0")
    conditioned, module = coin(device, data(n), "probs")
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=SEED, validate=True)
    optimizer = Adam(module.parameters(), lr=0.02)

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, {"theta": module()})
        loss.backward()
        optimizer.step()
        return loss

    if graph:
        # (the warm-up steps run eagerly and count: steps = warm-up + replays * repeat)
        replay = StepGraph(step, warmup=steps - 2, repeat=2)
        replay()
        replay.check()
    else:
        for _ in range(steps):
            step()
    torch.cuda.synchronize()
    assert loss_fn.last_fusions["particle_sums"] == 1
    return [p.detach().clone() for p in module.parameters()], dict(loss_fn.last_fusions)


def test_captured_steps_equal_eager_steps(device, monkeypatch):
    eager, _ = train(device, monkeypatch, True, 4)
    replayed, _ = train(device, monkeypatch, True, 4, graph=True)
    for a, b in zip(eager, replayed):
        assert torch.equal(a, b)


def test_adam_in_the_finish(device, monkeypatch):
    held, fusions = train(device, monkeypatch, True, 3)
    assert fusions["optimizer_step"] == 1
    apart, fusions = train(device, monkeypatch, False, 3)
    assert fusions["optimizer_step"] == 0
    for a, b in zip(held, apart):
        assert torch.equal(a, b)


def test_separate_reductions_take_the_per_particle_form(device, monkeypatch):
    x = data(20000)
    on = evaluate(device, monkeypatch, x, 1500, "probs", True)
    apart = evaluate(device, monkeypatch, x, 1500, "probs", True,
                     env=[("MININF_AMD_FUSE_REDUCE", "0")])
    for _, _, fusions in apart:
        assert fusions["particle_sums"] == 0 and fusions["deferred_reductions"] == 0
    check_against(on, apart)


def launcher_for(device, x, probs, K, per_site):
    n = x.numel()
    site = SiteRecord("x", "bernoulli_probs", [], torch.Size([n]), 1.0, None, "bernoulli_probs")
    views = [engine._View(probs, probs.stride(0), 0),
             engine._View(x.reshape(1, -1).expand(K, n), 0, x.stride(0))]
    launcher = engine._GroupLauncher(K, n, -1.0 / K, device, per_site=per_site)
    assert launcher.try_add(site, views, None)
    return launcher


def test_per_site_values_take_the_per_particle_form(device):
    """A launch that returns per-site values keeps them per particle; the same launch without
    them leaves doubles whose sum is the sum of those values. (Per-site values are a launcher
    option, engine._GroupLauncher(per_site=True): EvidenceLowerBoundLoss has no way to ask.)"""
    K, n = 1500, 20000
    x = data(n).to(device)
    gen = torch.Generator().manual_seed(5)
    probs = (0.1 + 0.8 * torch.rand(K, 1, generator=gen)).to(device).requires_grad_()
    wanted = launcher_for(device, x, probs, K, True)
    total, site_lp, _, _, _ = wanted.run(True, defer=True, ksum=True)
    assert wanted.reduce is not None and wanted.reduce.ksum == 0
    nat.check(nat.lib().mi_reduce_launch(ctypes.byref(wanted.reduce),
                                         nat.stream_handle(device)), "mi_reduce_launch")
    summed = launcher_for(device, x, probs, K, False)
    summed.run(True, defer=True, ksum=True)
    job = summed.reduce
    assert job is not None and job.ksum == 1 and job.nksum > 0
    # a job without per-particle values is never finalized on its own
    assert nat.lib().mi_reduce_launch(ctypes.byref(job), nat.stream_handle(device)) == \
        nat.MI_EUNSUPPORTED
    torch.cuda.synchronize()
    blocks = job.num_sites + job.num_slots - 1
    offset = (blocks * job.nseg * job.K * 4 + 255) // 256 * 256
    doubles = summed.workspace[offset:offset + 8 * job.nksum].view(torch.float64)
    want = site_lp.double().sum()
    print("sum of doubles", float(doubles.sum()), "sum of per-particle values", float(want))
    assert float(doubles.sum()) == pytest.approx(float(want), rel=1e-6)
    assert float(total.double().sum()) == pytest.approx(float(want), rel=1e-6)


@pytest.mark.parametrize("bad", ["data", "parameter"])
def test_validation_still_raises(device, monkeypatch, bad):
    n, K = 20000, 1500
    x = data(n)
    # a clean step of the same shape takes the particle-summed form
    clean = evaluate(device, monkeypatch, x, K, "probs", True, steps=1)
    assert clean[0][2]["particle_sums"] == 1
    if bad == "data":
        x[77] = 0.5
    conditioned, module = coin(device, x, "probs")
    if bad == "parameter":
        with torch.no_grad():
            next(iter(module.parameters())).fill_(float("nan"))
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=SEED)
    with pytest.raises(ValueError):
        loss_fn(conditioned, {"theta": module()})
