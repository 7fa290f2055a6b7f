"""
Several chunks per workgroup in the matrix launch of the Bernoulli BCAST kernel
(k_site_bcast_smem, MININF_AMD_BCAST_CPW): a workgroup that owns 2 or 4 consecutive chunks of its
particle block writes, for every chunk, what the workgroup of that chunk alone wrote. Every case
forces MININF_AMD_BCAST_CPW to 2 and to 4 and compares with MININF_AMD_BCAST_CPW=1 of the same
build, bit for bit.

Shapes: at K <= 2100 chunks hold 4096 elements, so n = 4097, 8200, 16392, 20000 are 2, 3, 5 and 5
chunks: a partial group under both settings, a one-element last chunk (4097), an eight-element one
(8200, 16392: a partial lane) and one with a partial fragment (20000: 3616 elements). K = 64 is one
wave, K = 1029 a second particle block with five particles in its first wave, K = 2100 three
particle blocks.

What a launch leaves in its workspace and what is compared (the rest of the workspace is never
written by these launches and holds whatever the allocator left): the [nseg, K] value rows (the
per-particle form), the slot's rank-one rows u[nseg], f[K], e[K] at the head of the slot's block
(nseg >= 3 and one slot: every case here), and the particle sums (one double per chunk and particle
block, then one per particle slot and block from four chunks on, else one per block).
"""
import pytest
import torch
from torch.distributions import Bernoulli, Beta

import mininf_amd as mi
from mininf_amd import engine
from mininf_amd.optim import Adam
from mininf_amd.particles import SiteRecord

SWITCHES = ("MININF_AMD_BCAST_SUFFSTAT", "MININF_AMD_BCAST_MFMA", "MININF_AMD_BCAST_CPW",
            "MININF_AMD_BCAST_KSUM", "MININF_AMD_FOLD_PRIOR", "MININF_AMD_BETA_SIDE")
SUFF = [("MININF_AMD_BCAST_SUFFSTAT", "1")]
OFF = [("MININF_AMD_BCAST_MFMA", "0")]
NS = [4097, 8200, 16392, 20000]
KS = [64, 1029, 2100]
CHUNK = 4096


@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
    """Later tests of the suite draw from torch's global generators without seeding them: this
    module leaves both where it found them."""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


def cpw(value):
    return [("MININF_AMD_BCAST_CPW", str(value))]


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


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def set_switches(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)


def launcher_for(device, family, a, x, per_site):
    K, N = a.numel(), x.numel()
    param = a.to(device).reshape(K, 1).clone().requires_grad_()
    views = [engine._View(param, param.stride(0), 0),
             engine._View(x.reshape(1, -1).expand(K, N), 0, x.stride(0))]
    site = SiteRecord("s", family, [], torch.Size([N]), 1.0, None, family)
    launcher = engine._GroupLauncher(K, N, -1.0, device, per_site=per_site)
    assert launcher.try_add(site, views, None)
    return launcher


def regions(workspace, K, chunks, gy, summed):
    """The written parts of a launch's workspace (module docstring), as raw int32 words."""
    nseg = chunks + 1
    words = workspace.view(torch.int32)
    block = nseg * K
    out = {}
    if not summed:
        out["values"] = words[:block]
    slot = 0 if summed else block
    out["rank-one rows"] = words[slot:slot + nseg + 2 * K]
    if summed:
        offset = (block * 4 + 255) // 256 * 256 // 4
        doubles = (chunks + (4 if chunks >= 4 else 1)) * gy
        out["particle sums"] = words[offset:offset + 2 * doubles]
    return out


def launch(monkeypatch, device, family, a, x, env=(), summed=False):
    """One Bernoulli site of per-particle parameters `a` [K] against shared data `x` [N] (a device
    tensor, possibly an offset view). Per particle: totals, slot gradient, flags and the workspace's
    written parts. `summed`: the launch leaves its values summed over particles (MI_GROUP_KSUM) and
    its reduction to the caller: flags and the workspace's written parts."""
    set_switches(monkeypatch, env)
    K, n = a.numel(), x.numel()
    chunks, gy = -(-n // CHUNK), -(-K // 1024)
    launcher = launcher_for(device, family, a, x, per_site=not summed)
    if summed:
        _, _, _, _, flags = launcher.run(True, defer=True, ksum=True)
        assert launcher.reduce is not None and launcher.reduce.ksum == 1
        assert launcher.reduce.nseg == chunks + 1
        out = {"flags": flags}
    else:
        total, _, _, slot, flags = launcher.run(True)
        out = {"total": total, "slot": slot, "flags": flags}
    torch.cuda.synchronize()
    set_switches(monkeypatch, ())
    out = {name: value.clone().cpu() for name, value in out.items()}
    out.update(regions(launcher.workspace.clone().cpu(), K, chunks, gy, summed))
    return out


def assert_same(got, want, names=None):
    for name in names or want:
        assert same_bits(got[name], want[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("summed", [True, False])
@pytest.mark.parametrize("family", ["bernoulli_probs", "bernoulli_logits"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_grouped_chunks_leave_the_same_bits(device, monkeypatch, family, K, n, summed):
    """Forced to 2 and to 4, and with the switch unset (these shapes fit one round: one chunk per
    workgroup), a launch leaves what MININF_AMD_BCAST_CPW=1 leaves; all equal the closed form."""
    x = binary(n).to(device)
    a = parameters(family, K)
    one = launch(monkeypatch, device, family, a, x, env=cpw(1), summed=summed)
    closed = launch(monkeypatch, device, family, a, x, env=SUFF, summed=summed)
    assert (one["flags"] == 0).all()
    assert_same(one, closed, ["flags"] if summed else ["total", "slot", "flags"])
    for env in (cpw(2), cpw(4), ()):
        got = launch(monkeypatch, device, family, a, x, env=env, summed=summed)
        assert_same(got, one)
        assert_same(got, closed, ["flags", "particle sums"] if summed else ["total", "slot", "flags"])


def value_rows(out, nseg, K):
    return out["values"].view(torch.float32).reshape(nseg, K)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks_per_workgroup", [2, 4])
@pytest.mark.parametrize("where", [1, 0, 2])
def test_a_chunk_with_another_value_in_a_group(device, monkeypatch, chunks_per_workgroup, where):
    """Three chunks, one of which holds a 0.5: that chunk's values equal MININF_AMD_BCAST_MFMA=0 bit
    for bit, the other chunks', in the same workgroup or the next, the closed form; the support
    flag is raised; everything written equals MININF_AMD_BCAST_CPW=1."""
    K, n, nseg = 1029, 8200, 4
    x = binary(n)
    x[where * CHUNK + (77 if where < 2 else 3)] = 0.5
    x = x.to(device)
    a = parameters("bernoulli_probs", K)
    got = launch(monkeypatch, device, "bernoulli_probs", a, x, env=cpw(chunks_per_workgroup))
    one = launch(monkeypatch, device, "bernoulli_probs", a, x, env=cpw(1))
    off = launch(monkeypatch, device, "bernoulli_probs", a, x, env=OFF)
    closed = launch(monkeypatch, device, "bernoulli_probs", a, x, env=SUFF)
    rows, rows_off, rows_closed = (value_rows(o, nseg, K) for o in (got, off, closed))
    assert same_bits(rows[where], rows_off[where])
    assert not same_bits(rows_off[where], rows_closed[where])   # (the comparison can tell them apart)
    for c in range(nseg):
        if c != where:
            assert same_bits(rows[c], rows_closed[c])
    assert bool((got["flags"] != 0).any())
    assert_same(got, one)
    assert_same(got, off, ["slot", "flags"])
    # The particle-summed form (the form the benchmark's launch takes): one double per chunk and
    # particle block, from the matrix chunks' sum round or from the scalar-load chunk's own.
    gy = 2
    summed = {name: launch(monkeypatch, device, "bernoulli_probs", a, x, env=env, summed=True)
              for name, env in (("got", cpw(chunks_per_workgroup)), ("one", cpw(1)), ("off", OFF),
                                ("closed", SUFF))}
    sums = {name: out["particle sums"].view(torch.float64)[:(nseg - 1) * gy].reshape(nseg - 1, gy)
            for name, out in summed.items()}
    assert torch.equal(sums["got"][where], sums["off"][where])
    assert not torch.equal(sums["off"][where], sums["closed"][where])
    for c in range(nseg - 1):
        if c != where:
            assert torch.equal(sums["got"][c], sums["closed"][c])
    assert bool((summed["got"]["flags"] != 0).any())
    assert_same(summed["got"], summed["one"])


@pytest.mark.gpu
@pytest.mark.parametrize("chunks_per_workgroup", [2, 4])
def test_a_replayed_grouped_launch_chooses_per_chunk_again(device, monkeypatch, chunks_per_workgroup):
    """Captured once and replayed with the 0.5 moved from chunk to chunk (and taken out), a grouped
    launch leaves at every replay what the eager MININF_AMD_BCAST_CPW=1 launch leaves on that
    data."""
    K, n, nseg = 1029, 8200, 4
    a = parameters("bernoulli_probs", K)
    clean = binary(n)
    x = clean.clone().to(device)
    set_switches(monkeypatch, cpw(chunks_per_workgroup))
    launcher = launcher_for(device, "bernoulli_probs", a, x, per_site=True)
    launcher.run(True)             # (eager once: nothing is built for the first time in the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, _, _, slot, flags = launcher.run(True)
    set_switches(monkeypatch, ())
    workspace = launcher.workspace
    for where in (1, 0, 2, None):
        data = clean.clone()
        if where is not None:
            data[where * CHUNK + 3] = 0.5
        x.copy_(data.to(device))
        workspace.zero_()
        flags.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = {"total": total.clone().cpu(), "slot": slot.clone().cpu(), "flags": flags.clone().cpu()}
        got.update(regions(workspace.clone().cpu(), K, nseg - 1, 2, False))
        want = launch(monkeypatch, device, "bernoulli_probs", a, data.to(device), env=cpw(1))
        assert_same(got, want)
        assert bool((got["flags"] != 0).any()) == (where is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["bernoulli_probs", "bernoulli_logits"])
def test_misaligned_data(device, monkeypatch, family):
    K, n = 1029, 8200
    x = binary(n + 1).to(device)[1:]
    assert x.data_ptr() % 16 == 4
    a = parameters(family, K)
    for summed in (False, True):
        got = launch(monkeypatch, device, family, a, x, env=cpw(2), summed=summed)
        one = launch(monkeypatch, device, family, a, x, env=cpw(1), summed=summed)
        assert_same(got, one)


def step_outputs(device, monkeypatch, x, K, env):
    """Four optimizer steps of the README model (Beta prior folded into the Bernoulli launch, the
    Beta guide's implicit-gradient factors as its side job): losses, parameters, gradients,
    last_fusions."""
    set_switches(monkeypatch, env)
    n = x.numel()

    def model():
        theta = mi.sample("theta", Beta(2, 2))
        mi.sample("x", Bernoulli(theta, validate_args=False), sample_shape=[n])

    module = mi.nn.ParameterizedDistribution(Beta, concentration1=1.5, concentration0=2.5).to(device)
    conditioned = mi.condition(model, x=x.to(device))
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=11, validate=False)
    optimizer = Adam(module.parameters(), lr=0.02)
    tensors = []
    for _ in range(4):
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, {"theta": module()})
        loss.backward()
        tensors.append(loss.detach().clone())
        tensors += [p.grad.detach().clone() for p in module.parameters()]
        optimizer.step()
        tensors += [p.detach().clone() for p in module.parameters()]
    torch.cuda.synchronize()
    set_switches(monkeypatch, ())
    return [t.cpu().reshape(-1) for t in tensors], dict(loss_fn.last_fusions)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 30000])
@pytest.mark.parametrize("extra", [(), (("MININF_AMD_FOLD_PRIOR", "0"),),
                                   (("MININF_AMD_BETA_SIDE", "0"),)])
def test_steps_with_the_folded_prior_and_the_side_job(device, monkeypatch, extra, n):
    """The particle-constant segment, the folded prior and the side job in front of the grid: four
    steps equal MININF_AMD_BCAST_CPW=1 in every loss, gradient and parameter, and fuse the same
    things. n = 20000 is 5 chunks, 3 or 2 chunk groups: group 0 evaluates every particle slot.
    n = 30000 is 8 chunks: four groups of two, slot s by group s (the benchmark's case), or two
    groups of four."""
    K = 1029
    x = binary(n)
    one = step_outputs(device, monkeypatch, x, K, list(extra) + cpw(1))
    for value in (2, 4):
        got = step_outputs(device, monkeypatch, x, K, list(extra) + cpw(value))
        assert len(got[0]) == len(one[0])
        for a, b in zip(got[0], one[0]):
            assert same_bits(a, b)
        assert got[1] == one[1]


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk", [(262144, 4096), (1_000_000, 3936)])
def test_the_automatic_choice_at_workload_size(device, monkeypatch, n, chunk):
    """K = 4096: 64 chunks x 4 particle blocks fit one round and keep one chunk per workgroup;
    n = 1e6 (255 chunks of 3936 x 4 blocks, the benchmark's launch) is grouped by the automatic
    choice, and leaves what MININF_AMD_BCAST_CPW=1 leaves. One launch per setting."""
    K = 4096
    x = binary(n).to(device)
    a = parameters("bernoulli_probs", K)
    chunks = -(-n // chunk)

    def run(env):
        set_switches(monkeypatch, env)
        launcher = launcher_for(device, "bernoulli_probs", a, x, per_site=False)
        _, _, _, _, flags = launcher.run(True, defer=True, ksum=True)
        assert launcher.reduce is not None and launcher.reduce.ksum == 1
        assert launcher.reduce.nseg == chunks + 1
        torch.cuda.synchronize()
        set_switches(monkeypatch, ())
        out = {"flags": flags.clone().cpu()}
        out.update(regions(launcher.workspace.clone().cpu(), K, chunks, 4, True))
        return out

    got, one = run(()), run(cpw(1))
    assert_same(got, one)
    sums = got["particle sums"].view(torch.float64)
    assert sums.numel() == (chunks + 4) * 4 and bool(torch.isfinite(sums).all())
