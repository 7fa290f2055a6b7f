"""
The int8 matrix loop of the Bernoulli BCAST kernel (k_site_bcast_smem): a 0 / 1 chunk is summed
with v_mfma_i32_16x16x64_i8 on three balanced base-256 digits of each logit's recentred fraction,
and the implicit leading one and the recentring constant enter through the chunk's count of ones:

    l = (-1)^s M 2^E,   M = f + (e > 0 ? 2^23 : 0),   E = max(e, 1) - 150,
    c = (e > 0 ? 2^23 : 0) + 2^22,   M - c = d0 + 256 d1 + 65536 d2,   d_q in [-128, 127],
    chunk total = (-1)^s (c n1 + D0 + 256 D1 + 65536 D2) 2^E = l n1      (D_q = d_q n1).

The logits here are built from bit patterns at the digit boundaries (carries between the digits,
the ends of the fraction, the extreme exponents, subnormals, both zeros), and every chunk row of a
launch must equal float32(float64(l) * count) bit for bit: the product is exact in fp64 (24 x 13
bits), so that is one rounding, the store's. Zeros are compared by value.

Shapes: family bernoulli_logits, K = 64 (one wave). At K <= 2048 a chunk holds 4096 elements and a
fragment 1024, so n = 1025 is a full fragment and one element, 3071 / 3073 a partial last fragment
and three fragments and one element, 4097 a whole chunk and a one-element chunk; 1024 is exactly one
fragment. n = 1023 is below the BCAST kernel's first size (N >= 1024: bcast_eligible) and runs the
column kernel, which no switch here touches and which has no chunk rows: it is kept so that the
boundary stays checked, against the closed-form launch only.
"""
import numpy as np
import pytest
import torch

from mininf_amd import engine
from mininf_amd.particles import SiteRecord

SWITCHES = ("MININF_AMD_BCAST_SUFFSTAT", "MININF_AMD_BCAST_MFMA", "MININF_AMD_BCAST_CPW",
            "MININF_AMD_BCAST_KSUM", "MININF_AMD_FOLD_PRIOR", "MININF_AMD_BETA_SIDE")
SUFF = [("MININF_AMD_BCAST_SUFFSTAT", "1")]
OFF = [("MININF_AMD_BCAST_MFMA", "0")]
CHUNK = 4096
K = 64
NS = [1023, 1024, 1025, 3071, 3073, 4097]

HALF = 1 << 22
FRACTIONS = [0, 1, 127, 128, 129, HALF - 129, HALF - 128, HALF - 1, HALF, HALF + 127, HALF + 128,
             (1 << 23) - 1,
             # d1 at +127 / -127 / -128 (with d0 at the same end)
             HALF + (127 * 256 + 127), HALF - (127 * 256 + 127), HALF - (128 * 256 + 128)]
# biased exponents: subnormals and zeros, 2^-126 (the least normal), 2^-60, 1, 2^60, 2^127 (up to
# FLT_MAX)
EXPONENTS = [0, 1, 67, 127, 187, 254]


def boundary_bits():
    bits = [(s << 31) | (e << 23) | f for e in EXPONENTS for f in FRACTIONS for s in (0, 1)]
    return np.array(bits, dtype=np.uint32)


BITS = boundary_bits()                    # 180 patterns, +0 and -0 among them
LOGITS = BITS.view(np.float32)
assert np.isfinite(LOGITS).all() and LOGITS.max() == np.finfo(np.float32).max
IN_RANGE = LOGITS[(np.abs(LOGITS) >= 2.0 ** -60) & (np.abs(LOGITS) <= 2.0 ** 60)]   # 62 of them
assert IN_RANGE.size == 62


def batches(values, size=K):
    """`values` in launches of `size` particles, the last one filled up with 1.0."""
    out = []
    for i in range(0, values.size, size):
        part = values[i:i + size]
        out.append(np.concatenate([part, np.ones(size - part.size, dtype=np.float32)]))
    return out


def digits(bits):
    """sign, c, the three digits and E of fp32 bit patterns (int64 arrays), as the kernel splits."""
    u = bits.astype(np.int64)
    s, e, f = u >> 31, (u >> 23) & 0xff, u & 0x7fffff
    lead = np.where(e > 0, 1 << 23, 0)
    M, c, E = f + lead, lead + HALF, np.maximum(e, 1) - 150
    r = M - c
    d = []
    for _ in range(3):
        dq = ((r & 0xff) ^ 0x80) - 0x80
        r = (r - dq) >> 8
        d.append(dq)
    assert (r == 0).all()
    return s, c, d, E, M


def test_the_digits_and_the_counts_are_exact():
    """The exactness argument restated on the host: over 5e5 random finite fp32 patterns and the
    boundary set, the digits are int8, c + d0 + 256 d1 + 65536 d2 is the significand, and
    (-1)^s (c n + sum_q 256^q d_q n) 2^E is l n in fp64."""
    rng = np.random.default_rng(23)
    bits = rng.integers(0, 1 << 32, size=500_000, dtype=np.uint64).astype(np.uint32)
    bits = bits[((bits >> 23) & 0xff) != 0xff]
    bits = np.concatenate([bits, BITS])
    s, c, d, E, M = digits(bits)
    for dq in d:
        assert dq.min() >= -128 and dq.max() <= 127
    assert (c + d[0] + 256 * d[1] + 65536 * d[2] == M).all()
    l = bits.view(np.float32).astype(np.float64)
    for n in (1, 3, 2755, 3936, 4095, 4096):
        D = [dq * n for dq in d]
        assert max(int(np.abs(Dq).max()) for Dq in D) <= 4096 * 128
        S = c * n + D[0] + 256 * D[1] + 65536 * D[2]
        assert int(S.max()) < 1 << 36 and int(S.min()) >= 0
        total = np.where(s == 1, -1.0, 1.0) * S.astype(np.float64) * np.ldexp(1.0, E.astype(np.int32))
        assert np.array_equal(total, l * n)


# ---- launches (the helpers of test_gpu_bcast_multichunk.py) --------------------------------------

@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
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


def parameters(K, seed=5):
    """Finite logits of magnitude in [2^-60, 2^60]."""
    gen = torch.Generator().manual_seed(seed + K)
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


def launcher_for(device, a, x, per_site):
    K, N = a.numel(), x.numel()
    param = a.to(device).reshape(K, 1).clone().requires_grad_()
    views = [engine._View(param, param.stride(0), 0),
             engine._View(x.reshape(1, -1).expand(K, N), 0, x.stride(0))]
    site = SiteRecord("s", "bernoulli_logits", [], torch.Size([N]), 1.0, None, "bernoulli_logits")
    launcher = engine._GroupLauncher(K, N, -1.0, device, per_site=per_site)
    assert launcher.try_add(site, views, None)
    return launcher


def regions(workspace, K, chunks, gy, summed):
    """The written parts of a launch's workspace, as raw int32 words: the [nseg, K] value rows
    (per-particle form), the slot's rank-one rows u[nseg], f[K], e[K] (nseg >= 3), the particle
    sums (summed form)."""
    nseg = chunks + 1
    words = workspace.view(torch.int32)
    block = nseg * K
    out = {}
    if not summed:
        out["values"] = words[:block]
    slot = 0 if summed else block
    if nseg >= 3:
        out["rank-one rows"] = words[slot:slot + nseg + 2 * K]
    if summed:
        offset = (block * 4 + 255) // 256 * 256 // 4
        doubles = (chunks + (4 if chunks >= 4 else 1)) * gy
        out["particle sums"] = words[offset:offset + 2 * doubles]
    return out


def launch(monkeypatch, device, a, x, env=(), summed=False):
    """One Bernoulli(logits) site of per-particle logits `a` [K] against shared data `x` [N] (a
    device tensor, possibly an offset view): totals, slot gradient, flags (per-particle form) or
    flags (summed form), and the workspace's written parts."""
    set_switches(monkeypatch, env)
    K, n = a.numel(), x.numel()
    chunks, gy = -(-n // CHUNK), -(-K // 1024)
    launcher = launcher_for(device, a, x, per_site=not summed)
    if summed:
        _, _, _, _, flags = launcher.run(True, defer=True, ksum=True)
        out = {"flags": flags}
    else:
        total, _, _, slot, flags = launcher.run(True)
        out = {"total": total, "slot": slot, "flags": flags}
    torch.cuda.synchronize()
    set_switches(monkeypatch, ())
    out = {name: value.clone().cpu() for name, value in out.items()}
    if n >= 1024:   # (below: the column kernel, another layout)
        out.update(regions(launcher.workspace.clone().cpu(), K, chunks, gy, summed))
    return out


def value_rows(out, nseg, K):
    return out["values"].view(torch.float32).reshape(nseg, K).numpy()


def counts_of(x, n):
    return [float(x[c * CHUNK:(c + 1) * CHUNK].sum()) for c in range(-(-n // CHUNK))]


def expected_row(l, count):
    """float32(float64(l) * count): exact product, one rounding (overflow to infinity included)."""
    with np.errstate(over="ignore"):
        return (l.astype(np.float64) * count).astype(np.float32)


def assert_rows_exact(rows, l, counts):
    for c, count in enumerate(counts):
        want, got = expected_row(l, count), rows[c]
        zero = want == 0
        assert np.array_equal(got[zero], want[zero])            # a zero of either sign
        assert np.array_equal(got[~zero].view(np.int32), want[~zero].view(np.int32)), (c, count)


DATA = {"binary": binary, "ones": lambda n: torch.ones(n), "zeros": lambda n: torch.zeros(n)}


@pytest.mark.gpu
@pytest.mark.parametrize("data", list(DATA))
@pytest.mark.parametrize("n", NS)
def test_digit_boundaries(device, monkeypatch, n, data):
    """Every chunk row is float32(l * count) bit for bit, subnormal logits included (no 2^-126
    allowance), on random 0 / 1 data and at the extreme counts: all ones (count = the chunk's
    length, D_q down to -2^19) and all zeros."""
    x = DATA[data](n)
    counts = counts_of(x, n)
    x = x.to(device)
    for l in batches(LOGITS):
        out = launch(monkeypatch, device, torch.from_numpy(l), x)
        assert (out["flags"] == 0).all()
        if n >= 1024:
            assert_rows_exact(value_rows(out, len(counts) + 1, K), l, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("data", list(DATA))
@pytest.mark.parametrize("n", NS)
def test_boundaries_equal_the_closed_form(device, monkeypatch, n, data):
    """Logits of magnitude in [2^-60, 2^60]: totals, slot gradients and flags equal
    MININF_AMD_BCAST_SUFFSTAT=1 bit for bit, and a second launch equals the first."""
    x = DATA[data](n).to(device)
    (l,) = batches(IN_RANGE)
    a = torch.from_numpy(l)
    got = launch(monkeypatch, device, a, x)
    again = launch(monkeypatch, device, a, x)
    closed = launch(monkeypatch, device, a, x, env=SUFF)
    for name in ("total", "slot", "flags"):
        assert same_bits(got[name], closed[name]), name
    for name in got:
        assert same_bits(got[name], again[name]), name
    assert (got["flags"] == 0).all()
    assert bool(torch.isfinite(got["total"]).all())


def grouped_case():
    """K = 1029 (a second particle block with five particles in its first wave), n = 3 * 4096 + 8:
    four chunks, chunk 1 with a 0.3 in it. The logits: the whole boundary set, then random ones."""
    K2, n = 1029, 3 * CHUNK + 8
    x = binary(n)
    x[CHUNK + 77] = 0.3
    a = torch.cat([torch.from_numpy(LOGITS.copy()), parameters(K2 - LOGITS.size)])
    return K2, n, x, a


@pytest.mark.gpu
@pytest.mark.parametrize("summed", [False, True])
def test_several_chunks_per_workgroup(device, monkeypatch, summed):
    """MININF_AMD_BCAST_CPW = 1, 2 and 4 leave the same value rows, rank-one rows and particle
    sums bit for bit, with the scalar-load loop running inside a grouped workgroup (the chunk with
    the 0.3); the 0 / 1 chunks' rows are float32(l * count) at every setting."""
    K2, n, x, a = grouped_case()
    counts = counts_of(x, n)
    x = x.to(device)
    one = launch(monkeypatch, device, a, x, env=cpw(1), summed=summed)
    assert bool((one["flags"] != 0).any())
    outs = [one] + [launch(monkeypatch, device, a, x, env=cpw(v), summed=summed) for v in (2, 4)]
    for got in outs[1:]:
        assert set(got) == set(one)
        for name in one:
            assert same_bits(got[name], one[name]), name
    if not summed:
        off = launch(monkeypatch, device, a, x, env=OFF)
        for got in outs:
            rows = value_rows(got, 5, K2)
            assert same_bits(torch.from_numpy(rows[1]), torch.from_numpy(value_rows(off, 5, K2)[1]))
            keep = [0, 2, 3]
            assert_rows_exact(rows[keep], a.numpy(), [counts[c] for c in keep])


@pytest.mark.gpu
@pytest.mark.parametrize("summed", [False, True])
@pytest.mark.parametrize("other", [100.0, -1.0, float("nan")])
def test_a_large_sum_next_to_binary_chunks(device, monkeypatch, other, summed):
    """Chunk 0 holds `other` throughout, so its sum (409600, -4096, NaN) is no count and fits no
    16-bit field; chunks 1 to 3 of the same workgroup (two and two at MININF_AMD_BCAST_CPW=2, all
    four at 4) are 0 / 1. Their counts must not be touched by it: their rows are float32(l * count)
    at every setting, and everything written equals MININF_AMD_BCAST_CPW=1 bit for bit."""
    K2, n = 1029, 3 * CHUNK + 8
    x = binary(n)
    x[:CHUNK] = other
    counts = counts_of(x, n)
    a = torch.cat([torch.from_numpy(LOGITS.copy()), parameters(K2 - LOGITS.size)])
    x = x.to(device)
    one = launch(monkeypatch, device, a, x, env=cpw(1), summed=summed)
    assert bool((one["flags"] != 0).any())
    outs = [one] + [launch(monkeypatch, device, a, x, env=cpw(v), summed=summed) for v in (2, 4)]
    for got in outs[1:]:
        assert set(got) == set(one)
        for name in one:
            assert same_bits(got[name], one[name]), name
    if not summed:
        keep = [1, 2, 3]
        for got in outs:
            assert_rows_exact(value_rows(got, 5, K2)[keep], a.numpy(), [counts[c] for c in keep])


@pytest.mark.gpu
def test_misaligned_data(device, monkeypatch):
    """x one element off 16-byte alignment: the chunk image is written one element at a time."""
    K2, n = 1029, 8200
    host = binary(n + 1)
    x = host.to(device)[1:]
    assert x.data_ptr() % 16 == 4
    inside = torch.cat([torch.from_numpy(IN_RANGE.copy()), parameters(K2 - IN_RANGE.size)])
    got = launch(monkeypatch, device, inside, x)
    closed = launch(monkeypatch, device, inside, x, env=SUFF)
    for name in ("total", "slot", "flags"):
        assert same_bits(got[name], closed[name]), name
    a = torch.cat([torch.from_numpy(LOGITS.copy()), parameters(K2 - LOGITS.size)])
    out = launch(monkeypatch, device, a, x)
    assert_rows_exact(value_rows(out, 4, K2), a.numpy(), counts_of(host[1:], n))
