"""
The matrix loop of the Bernoulli BCAST kernel (k_site_bcast_smem, MININF_AMD_BCAST_MFMA): chunks
whose data is all 0 / 1 are summed on the bf16 matrix cores from three exact bf16 pieces of each
logit, so the default path equals the closed form l_k * sum_i x_i (MININF_AMD_BCAST_SUFFSTAT=1) bit
for bit; a chunk holding any other value takes the scalar-load loop and equals
MININF_AMD_BCAST_MFMA=0 bit for bit.

Shapes: the BCAST kernel exists from N = 1024 and K = 64 (bcast_eligible); smaller cases run the
column kernel, which neither switch touches, and are here so that the boundary stays checked. At
K <= 2048 chunks hold 4096 elements, so n = 4097 is a whole chunk and a one-element chunk, 8200 two
chunks and 8 elements; 1535 / 1537 / 2047 are one chunk with a partial last fragment (512 elements)
or a partial lane (16 elements). K = 1029 leaves five particles in the second block's first wave,
K = 64 one wave.

The float64 bound is the one of test_gpu_kernels.test_bcast_bernoulli_kernels (rtol 1e-6, atol
1e-6 N).
"""
import numpy as np
import pytest
import torch
from torch.distributions import Bernoulli, Beta, Normal

import mininf_amd as mi
from mininf_amd import engine
from mininf_amd.graph import StepGraph
from mininf_amd.optim import Adam
from mininf_amd.particles import SiteRecord

KS = [1, 33, 64, 1029]
NS = [10, 511, 513, 1535, 1537, 2047, 4097, 8200]


def binary(n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=gen) < 0.3).float()


def parameters(family, K, seed=5):
    """Finite logits of magnitude in [2^-60, 2^60] (probabilities whose logits are)."""
    gen = torch.Generator().manual_seed(seed + K)
    if family == "bernoulli_probs":
        return 0.01 + 0.98 * torch.rand(K, generator=gen)
    sign = torch.where(torch.rand(K, generator=gen) < 0.5, -1.0, 1.0)
    mag = torch.exp2(120 * torch.rand(K, generator=gen) - 60)
    mixed = torch.where(torch.arange(K) % 2 == 0, 3 * torch.randn(K, generator=gen), sign * mag)
    return mixed.clamp(-2.0 ** 60, 2.0 ** 60).float()


def launch(monkeypatch, device, family, a, x, env=()):
    """One Bernoulli site of per-particle parameters `a` [K] against shared data `x` [N] (a device
    tensor, possibly an offset view): per-particle totals, slot gradient, flags."""
    for name in ("MININF_AMD_BCAST_SUFFSTAT", "MININF_AMD_BCAST_MFMA"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    K, N = a.numel(), x.numel()
    param = a.to(device).reshape(K, 1).clone().requires_grad_()
    views = [engine._View(param, param.stride(0), 0),
             engine._View(x.reshape(1, -1).expand(K, N), 0, x.stride(0))]
    site = SiteRecord("s", family, [], torch.Size([N]), 1.0, None, family)
    launcher = engine._GroupLauncher(K, N, -1.0, device, per_site=True)
    assert launcher.try_add(site, views, None)
    total, _, _, slot, flags = launcher.run(True)
    torch.cuda.synchronize()
    for name, _ in env:
        monkeypatch.delenv(name)
    launch.workspace = launcher.workspace.clone().cpu()   # (the partials are still in it)
    return total.cpu(), slot.cpu(), flags.cpu()


def float64_totals(family, a, x):
    a, x = a.double(), x.double().cpu()
    logits = torch.log(a) - torch.log1p(-a) if family == "bernoulli_probs" else a
    softplus = torch.clamp(logits, min=0) + torch.log1p(torch.exp(-logits.abs()))
    return logits * x.sum() - x.numel() * softplus


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


SUFF = [("MININF_AMD_BCAST_SUFFSTAT", "1")]
OFF = [("MININF_AMD_BCAST_MFMA", "0")]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["bernoulli_probs", "bernoulli_logits"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_binary_data_equals_the_closed_form(device, monkeypatch, family, K, n):
    x = binary(n).to(device)
    a = parameters(family, K)
    total, slot, flags = launch(monkeypatch, device, family, a, x)
    again = launch(monkeypatch, device, family, a, x)
    closed = launch(monkeypatch, device, family, a, x, env=SUFF)
    for got, rerun, want in zip((total, slot, flags), again, closed):
        assert same_bits(got, want)
        assert same_bits(got, rerun)   # determinism
    assert (flags == 0).all()
    want = float64_totals(family, a, x)
    err = (total.double() - want).abs()
    print("largest error against float64", float(err.max()))
    assert bool((err <= 1e-6 * want.abs() + 1e-6 * n).all())


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["bernoulli_probs", "bernoulli_logits"])
def test_misaligned_data(device, monkeypatch, family):
    K, n = 1029, 8200
    x = binary(n + 1).to(device)[1:]
    assert x.data_ptr() % 16 == 4
    a = parameters(family, K)
    got = launch(monkeypatch, device, family, a, x)
    closed = launch(monkeypatch, device, family, a, x, env=SUFF)
    for g, w in zip(got, closed):
        assert same_bits(g, w)
    want = float64_totals(family, a, x)
    assert bool(((got[0].double() - want).abs() <= 1e-6 * want.abs() + 1e-6 * n).all())


def chunk_rows(nseg, K):
    """The [nseg, K] fp32 value block of the last launch: row c is chunk c's sum_i x_i l_k alone
    (the particle-constant part is the last row)."""
    return launch.workspace[:nseg * K * 4].view(torch.float32).reshape(nseg, K)


@pytest.mark.gpu
def test_tiny_and_non_finite_logits(device, monkeypatch):
    """|l| < 2^-100, mantissas drawn at random so that the second and third bf16 pieces are
    nonzero and, from about 2^-110 down, below bf16's normal range: each chunk's partial agrees
    with float64 l_k * (the chunk's count) within (the chunk's length) * 2^-126 on the matrix loop.
    The scalar-load loop (MININF_AMD_BCAST_MFMA=0) adds in fp32 and cannot meet that at the top of
    the range (measured 1.7e-34 against 4.8e-35 at |l| near 2^-101, ordinary rounding, no flush):
    its bound adds the rounding of its sums, chains of at most 64 fp32 terms carried in fp64 and
    one fp32 store, (64 + 1) * 2^-24 * |l_k| * count -- some 1e5 times smaller than the value, so
    a flushed logit still fails it."""
    K, n, nseg = 64, 4097, 3
    x = binary(n)
    x[4096] = 1.0                  # (the one-element chunk counts)
    counts = [float(x[:4096].sum()), float(x[4096:].sum())]
    lens = [4096, 1]
    x = x.to(device)
    gen = torch.Generator().manual_seed(17)
    a = torch.full((K,), 0.25)
    a[:32] = (1 + torch.rand(32, generator=gen)) * torch.exp2(-101 - torch.arange(32).float())
    a[32:40] = -a[:32:4]
    assert bool((a[:40].abs() < 2.0 ** -100).all()) and bool((a[:40] != 0).all())
    for env in ((), OFF):
        launch(monkeypatch, device, "bernoulli_logits", a, x, env=env)
        rows = chunk_rows(nseg, K)
        for c in (0, 1):
            want = a[:40].double() * counts[c]
            err = (rows[c, :40].double() - want).abs()
            bound = torch.full_like(want, lens[c] * 2.0 ** -126)
            if env:
                bound = bound + 65 * 2.0 ** -24 * want.abs()
            print("tiny logits", env, "chunk", c, "largest error", float(err.max()),
                  "bound", float(bound.min()), "largest value", float(want.abs().max()))
            assert bool((err <= bound).all())
    for bad in (float("nan"), float("inf"), float("-inf")):
        b = a.clone()
        b[40] = bad
        for env in ((), OFF):
            total, _, _ = launch(monkeypatch, device, "bernoulli_logits", b, x, env=env)
            assert not bool(torch.isfinite(total[40]))
            if bad != bad:
                assert bool(torch.isnan(total[40]))
            assert bool(torch.isfinite(total[41:]).all()) and bool(torch.isfinite(total[:40]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["bernoulli_probs", "bernoulli_logits"])
def test_other_values_take_the_scalar_loop(device, monkeypatch, family):
    """The path is chosen per workgroup, so in a launch of three chunks of which the second holds a
    0.3, that chunk's partial values equal MININF_AMD_BCAST_MFMA=0 bit for bit and the other two
    chunks' the closed form; the slot gradient, which no loop feeds, and the flags equal
    MININF_AMD_BCAST_MFMA=0 throughout. (The per-particle totals add the three chunks, so against
    MININF_AMD_BCAST_MFMA=0 they keep the float64 bound, not the bits.)"""
    K, n, nseg = 1029, 8200, 4
    x = binary(n)
    x[4096 + 77] = 0.3
    x = x.to(device)
    a = parameters(family, K)

    def run(env):
        out = launch(monkeypatch, device, family, a, x, env=env)
        return out, chunk_rows(nseg, K)

    got, rows = run(())
    off, rows_off = run(OFF)
    closed, rows_closed = run(SUFF)
    assert same_bits(rows[1], rows_off[1])
    assert not same_bits(rows_off[1], rows_closed[1])      # (the comparison can tell them apart)
    for c in (0, 2, 3):
        assert same_bits(rows[c], rows_closed[c])
    assert same_bits(got[1], off[1]) and same_bits(got[2], off[2])
    assert bool((got[2] != 0).any())    # the support flag
    assert bool(((got[0].double() - off[0].double()).abs()
                 <= 1e-6 * off[0].double().abs() + 1e-6 * n).all())
    clean = launch(monkeypatch, device, family, a, binary(n).to(device))
    assert (clean[2] == 0).all()


def replayed_launch(monkeypatch, device, family, a, x, env=()):
    """The launch of `launch`, captured into a graph and replayed twice: the chunk rows and the
    flags the replay left."""
    for name in ("MININF_AMD_BCAST_SUFFSTAT", "MININF_AMD_BCAST_MFMA"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    K, N = a.numel(), x.numel()
    param = a.to(device).reshape(K, 1).clone().requires_grad_()
    views = [engine._View(param, param.stride(0), 0),
             engine._View(x.reshape(1, -1).expand(K, N), 0, x.stride(0))]
    site = SiteRecord("s", family, [], torch.Size([N]), 1.0, None, family)
    launcher = engine._GroupLauncher(K, N, -1.0, device, per_site=True)
    assert launcher.try_add(site, views, None)
    launcher.run(True)             # (eager once: nothing is built for the first time in the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, _, _, slot, flags = launcher.run(True)
    workspace = launcher.workspace
    workspace.zero_()
    flags.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for name, _ in env:
        monkeypatch.delenv(name)
    return workspace.clone().cpu(), flags.clone().cpu(), slot.clone().cpu()


@pytest.mark.gpu
def test_a_replayed_launch_chooses_per_chunk_again(device, monkeypatch):
    """Captured and replayed, the launch of test_other_values_take_the_scalar_loop leaves the same
    rows: the chunk with the 0.3 equal to MININF_AMD_BCAST_MFMA=0 bit for bit, the others equal to
    the closed form, the slot gradient and the raised support flag equal to
    MININF_AMD_BCAST_MFMA=0."""
    K, n, nseg = 1029, 8200, 4
    x = binary(n)
    x[4096 + 77] = 0.3
    x = x.to(device)
    a = parameters("bernoulli_probs", K)

    def rows_of(workspace):
        return workspace[:nseg * K * 4].view(torch.float32).reshape(nseg, K)

    got = replayed_launch(monkeypatch, device, "bernoulli_probs", a, x)
    off = replayed_launch(monkeypatch, device, "bernoulli_probs", a, x, env=OFF)
    closed = replayed_launch(monkeypatch, device, "bernoulli_probs", a, x, env=SUFF)
    assert same_bits(rows_of(got[0])[1], rows_of(off[0])[1])
    assert not same_bits(rows_of(off[0])[1], rows_of(closed[0])[1])
    for c in (0, 2, 3):
        assert same_bits(rows_of(got[0])[c], rows_of(closed[0])[c])
    assert same_bits(got[1], off[1]) and bool((got[1] != 0).any())
    assert same_bits(got[2], off[2])
    launch(monkeypatch, device, "bernoulli_probs", a, x)
    assert same_bits(rows_of(got[0]), chunk_rows(nseg, K))   # (and equal to the eager launch)


def coin(device, x, form, prior=True):
    n = x.numel()
    if form == "probs":
        def model():
            theta = mi.sample("theta", Beta(2, 2))
            mi.sample("x", Bernoulli(theta, validate_args=False), sample_shape=[n])
        module = mi.nn.ParameterizedDistribution(Beta, concentration1=1.5,
                                                 concentration0=2.5).to(device)
    else:
        def model():
            z = mi.sample("theta", Normal(0.0, 1.0))
            mi.sample("x", Bernoulli(logits=z, validate_args=False), sample_shape=[n])
        module = mi.nn.ParameterizedDistribution(Normal, loc=-0.4, scale=0.3).to(device)
    return mi.condition(model, x=x.to(device)), module


def step_outputs(device, monkeypatch, x, K, form, env, graph=False):
    for name in ("MININF_AMD_BCAST_SUFFSTAT", "MININF_AMD_BCAST_MFMA", "MININF_AMD_BCAST_KSUM",
                 "MININF_AMD_FOLD_PRIOR", "MININF_AMD_ELBO_EXTERNAL"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    conditioned, module = coin(device, x, form)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=11, validate=False)
    optimizer = Adam(module.parameters(), lr=0.02)
    losses = []

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, {"theta": module()})
        loss.backward()
        optimizer.step()
        return loss

    if graph:
        replay = StepGraph(step, warmup=2, repeat=2)
        replay()
        replay.check()
    else:
        for _ in range(4):
            losses.append(step().detach().clone())
    torch.cuda.synchronize()
    for name, _ in env:
        monkeypatch.delenv(name)
    return losses, [p.detach().clone() for p in module.parameters()], dict(loss_fn.last_fusions)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["probs", "logits"])
@pytest.mark.parametrize("extra", [(), (("MININF_AMD_FOLD_PRIOR", "0"),),
                                   (("MININF_AMD_BCAST_KSUM", "0"),),
                                   (("MININF_AMD_ELBO_EXTERNAL", "1"),)])
def test_steps_equal_the_closed_form_and_keep_their_fusions(device, monkeypatch, form, extra):
    """Four optimizer steps, with and without the folded prior, particle-summed (MI_GROUP_KSUM),
    per particle, and with the reductions forced into launches of their own: losses and parameters
    equal the closed form's bit for bit, and last_fusions reads as with the matrix loop off."""
    K, n = 1500, 12321
    x = binary(n)
    got = step_outputs(device, monkeypatch, x, K, form, list(extra))
    closed = step_outputs(device, monkeypatch, x, K, form, list(extra) + SUFF)
    off = step_outputs(device, monkeypatch, x, K, form, list(extra) + OFF)
    for a, b in zip(got[0] + got[1], closed[0] + closed[1]):
        assert same_bits(a, b)
    assert got[2] == off[2] == closed[2]
    for a, b in zip(got[1], off[1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_a_replayed_step_with_other_values_equals_the_eager_one(device, monkeypatch):
    """The choice is made on the device, so a captured step makes it again at every replay: the
    replayed steps equal the eager ones bit for bit, and MININF_AMD_BCAST_MFMA=0 (which differs in
    the rounding of the chunks that are 0/1) within the bound of the particle-sum tests."""
    K, n = 1500, 12321
    x = binary(n)
    x[4096 + 5] = 0.3
    eager = step_outputs(device, monkeypatch, x, K, "probs", [])
    replayed = step_outputs(device, monkeypatch, x, K, "probs", [], graph=True)
    off = step_outputs(device, monkeypatch, x, K, "probs", OFF, graph=True)
    for a, b, c in zip(eager[1], replayed[1], off[1]):
        assert same_bits(a, b)
        torch.testing.assert_close(b, c, rtol=1e-5, atol=1e-6)


def test_the_split_and_the_counts_are_exact():
    """The exactness argument on the host: a finite fp32 logit is the sum of three bfloat16
    pieces, and a count of at most 4096 times a piece is exact in fp32."""
    gen = torch.Generator().manual_seed(0)
    logits = torch.cat([3 * torch.randn(200_000, generator=gen),
                        torch.log(torch.rand(200_000, generator=gen)),
                        torch.exp2(120 * torch.rand(50_000, generator=gen) - 60),
                        -torch.exp2(-100 * torch.rand(50_000, generator=gen))]).float()
    logits = logits[torch.isfinite(logits) & (logits != 0)]
    h = logits.bfloat16().float()
    m = (logits - h).bfloat16().float()
    lo = (logits - h - m).bfloat16().float()
    assert torch.equal(h.double() + m.double() + lo.double(), logits.double())
    for count in (1, 3, 2755, 3936, 4095, 4096):
        for piece in (h, m, lo):
            product = piece * float(count)                      # fp32
            assert torch.equal(product.double(), piece.double() * count)
    total = (h.double() + m.double() + lo.double()) * 3936
    assert torch.equal(total, logits.double() * 3936)
