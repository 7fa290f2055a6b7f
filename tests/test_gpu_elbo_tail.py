"""
The ELBO tail kernels (csrc/elbo.hip: mi_elbo_forward, mi_elbo_backward) descriptor by descriptor
against the float64 contract of tests/elbo_reference.py: terms and entropies, absorbed draws,
deferred reductions (in the launch and as launches of their own) and the argument checks. Every
output is pre-filled with NaN and compared whole; the bound of each quantity is
  2^-24 |want| + C_family 2^-24 (magnitude of its fp32 terms) + 1e-12 (sum of |fp64 summands|)
plus what elbo_reference adds for particular paths.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from mininf_amd import _native as nat
from tests import elbo_reference as ref
from tests import implicit_grad_cases as cases

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float("nan")

# C_family: 4x the largest err / (2^-24 magnitude) measured on the MI355X against the float64
# reference (the measurement beside each constant; every test prints its own). Caps: 16 for Gamma
# and Beta (a handful of fp32 operations of a few ulp each, the CPU restatement sits below 2) and
# for the Normal gradient (one division), 64 for the Normal entropy value (a lane adds up to about
# 32 logs in float before widening).
CAPS = {("value", "normal"): 64.0, ("value", "gamma"): 16.0, ("value", "beta"): 16.0,
        ("gradient", "normal"): 16.0, ("gradient", "gamma"): 16.0, ("gradient", "beta"): 16.0}
CONSTANTS = {("value", "normal"): 6.62,       # measured 1.655
             ("value", "gamma"): 1.584,       # measured 0.396
             ("value", "beta"): 0.776,        # measured 0.194
             ("gradient", "normal"): 3.444,   # measured 0.861
             ("gradient", "gamma"): 3.16,     # measured 0.790
             ("gradient", "beta"): 10.112}    # measured 2.528
MEASURED = {}


def _constants(kind):
    return {family: CONSTANTS[(kind, family)] for family in ref.FAMILIES}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nELBO tail, largest err / (2^-24 magnitude) by (kind, family):",
          {k: round(v, 3) for k, v in sorted(MEASURED.items())})


def test_constants_fit_their_caps():
    for key, value in CONSTANTS.items():
        assert value <= CAPS[key], key


def check(what, got, q, kind="value", rounding=True):
    """got against q at its bound; records the share of the error the family constant must cover,
    over 2^-24 times the family's magnitude (elements that one family alone has a part in)."""
    got = np.asarray(got, np.float64).reshape(q.value.shape)
    err = np.abs(got - q.value)
    consts = _constants(kind)
    bnd = ref.bound(q, consts, rounding)
    live = [k for k, m in q.mag.items() if np.any(m > 0)]
    for family in live:
        mag = q.mag[family]
        alone = mag > 0
        for other in live:
            if other != family:
                alone &= q.mag[other] == 0
        if alone.any():
            rest = ref.bound(q, dict.fromkeys(ref.FAMILIES, 0.0), rounding)
            ratio = (np.maximum(err - rest, 0.0)[alone] / (ref.EPS32 * mag[alone])).max()
            MEASURED[(kind, family)] = max(MEASURED.get((kind, family), 0.0), float(ratio))
    finite = np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        excess = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    print(f"{what}: worst {np.nanmax(np.where(finite, excess, np.inf)):.3g} of the bound")
    bad = ~finite | (err > bnd)
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], q.value[bad][:5], bnd[bad][:5])


# ---- one helper to build and launch --------------------------------------------------------------

def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


class Launch:
    """An nat.Elbo built from a case dict (tests/elbo_reference.py), its device arrays and its
    outputs, every one pre-filled with NaN."""

    def __init__(self, case, device, options=0, counters=False, nflags=0):
        self.case, self.device, self.keep = case, device, []
        self.lib = nat.lib()
        E = self.E = nat.Elbo()
        K = case["K"]
        E.K, E.g0, E.entropy_scale, E.options = K, float(case["g0"]), case["entropy_scale"], options
        for t, x in enumerate(case.get("terms", [])):
            E.terms[t] = self.dev(x).data_ptr()
        E.num_terms = len(case.get("terms", []))
        self.jobs = [self._job(j, job) for j, job in enumerate(case.get("jobs", []))]
        E.num_reduce = len(self.jobs)
        self.grads, self.saved = [], []
        for j, f in enumerate(case.get("factors", [])):
            self._factor(j, f)
        E.num_factors = len(case.get("factors", []))
        self.buffers = [self.dev(b) for b in case.get("buffers", [])]
        for b, x in enumerate(self.buffers):
            E.buffers[b], E.buffer_len[b] = max(x.data_ptr(), 8), x.numel()   # (empty: any address)
        E.num_buffers = len(self.buffers)
        self.counter = self.snapshot = self.flags = self.mirror = None
        if counters:
            self.counter = torch.tensor([41], dtype=torch.int64, device=device)
            self.snapshot = torch.tensor([-1], dtype=torch.int64, device=device)
            E.step_counter, E.step_snapshot = self.counter.data_ptr(), self.snapshot.data_ptr()
        if nflags:
            self.flags = torch.arange(3, 3 + nflags, dtype=torch.int32, device=device)
            self.mirror = torch.full((nflags,), -1, dtype=torch.int32, device=device)
            E.flags, E.flags_mirror, E.nflags = self.flags.data_ptr(), self.mirror.data_ptr(), nflags
        self.loss = torch.full((), NAN, device=device)
        self.dterm = torch.full((1,), NAN, device=device)
        size = ctypes.c_size_t()
        self.size_code = self.lib.mi_elbo_workspace_bytes(ctypes.byref(E), ctypes.byref(size))
        self.size = size.value
        self.ws = torch.full((max(self.size, nat.ELBO_COUNTER_BYTES),), 0xFF, dtype=torch.uint8,
                             device=device)
        self.stream = nat.stream_handle(device)
        nat.check(self.lib.mi_elbo_workspace_init(self.ws.data_ptr(), self.ws.numel(), self.stream),
                  "mi_elbo_workspace_init")

    def dev(self, x, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(x), device=self.device)
        if dtype is not None:
            t = t.to(dtype)
        self.keep.append(t)
        return t

    def nans(self, shape, dtype=torch.float32):
        t = torch.full(shape, NAN, dtype=dtype, device=self.device)
        self.keep.append(t)
        return t

    def _strided(self, values, stride, offset):
        """values at buf[offset + i * stride], NaN everywhere else; the address of element 0."""
        n = len(values)
        buf = np.full(offset + max(1, (n - 1) * stride + 1), np.nan, f32)
        if stride == 0:
            buf[offset] = values[0]
        else:
            buf[offset:offset + (n - 1) * stride + 1:stride] = values
        return self.dev(buf).data_ptr() + 4 * offset

    def _job(self, j, job):
        K, nseg, ns, nl = self.case["K"], job["nseg"], job["num_sites"], job["num_slots"]
        blocks = len(job["values"])
        ksum = job.get("ksum")
        floats = blocks * nseg * K
        off = (floats * 4 + 255) // 256 * 256
        part = np.full(off // 4 + (2 * ksum.size if ksum is not None else 0), np.nan, f32)
        rank1 = 0
        for b, v in enumerate(job["values"]):
            block = part[b * nseg * K:(b + 1) * nseg * K]
            if isinstance(v, dict):
                assert nseg + 2 * K <= nseg * K
                rank1 |= 1 << (b + (ns if ksum is not None else 0))
                block[:nseg], block[nseg:nseg + K], block[nseg + K:nseg + 2 * K] = v["u"], v["f"], v["e"]
            else:
                block[:] = np.asarray(v, f32).ravel()
        if ksum is not None:
            part[off // 4:] = np.ascontiguousarray(ksum, np.float64).ravel().view(f32)
        r = self.E.reduce[j]
        r.part, r.nseg, r.K, r.num_sites, r.num_slots = self.dev(part).data_ptr(), nseg, K, ns, nl
        r.rank1 = rank1
        for v in range(ns):
            r.scale[v] = job["scale"][v]
        r.slot_scale = job["slot_scale"]
        out = {"total": self.nans((K,)), "slot_grad": self.nans((max(1, nl), K)),
               "site_lp": self.nans((ns, K), torch.float64) if job.get("site_lp") else None}
        r.total, r.slot_grad = out["total"].data_ptr(), out["slot_grad"].data_ptr()
        r.site_lp = nat.ptr(out["site_lp"])
        if ksum is not None:
            r.ksum, r.nksum = (1 << ns) - 1, ksum.shape[1]
        return out

    def _factor(self, j, f):
        K, n, st = self.case["K"], f["n"], f.get("storage", {})
        d = self.E.factors[j]
        d.family = {"normal": nat.NORMAL, "gamma": nat.GAMMA, "beta": nat.BETA}[f["family"]]
        d.n, d.weight = n, f["weight"]
        if st.get("interleaved"):
            base = self.dev(np.stack([f["p0"], f["p1"]], 1)).data_ptr()
            d.param[0], d.param[1] = base, base + 4
            d.stride[0] = d.stride[1] = 2
        else:
            stride, offset = st.get("stride", (1, 1)), st.get("offset", (0, 0))
            for q, key in enumerate(("p0", "p1")):
                if f.get(key) is not None:
                    d.param[q] = self._strided(f[key], stride[q], offset[q])
                    d.stride[q] = stride[q]
        gs, gnull = st.get("grad_stride", (1, 1)), st.get("grad_null", (False, False))
        grads = []
        for q in range(2):
            g = None if gnull[q] else self.nans((max(1, (n - 1) * gs[q] + 1),))
            d.grad[q], d.grad_stride[q], d.transform[q] = nat.ptr(g), gs[q], f["transform"][q]
            grads.append(g)
        self.grads.append((grads, gs))
        saved = None
        kind = f.get("draw")
        if kind == "partials":
            d.draw_kind = nat.DRAW_PARTIALS
            d.partial[0], d.partial[1] = (self.dev(p).data_ptr() for p in f["partial"])
            d.partial_rows = f["partial"][0].shape[0]
        elif kind == "sources":
            d.draw_kind = nat.DRAW_SOURCES
            s = 0
            for job, slot in f.get("slot_sources", []):   # rows of a job's slot gradients
                d.source[s].ptr = self.jobs[job]["slot_grad"].data_ptr() + 4 * slot * K
                d.source[s].stride_k, d.source[s].stride_i = 1, (K if n > 1 else 0)
                s += 1
            layouts = f.get("source_layout", [])
            for q, x in enumerate(f.get("outside", f["sources"] if not f.get("slot_sources") else [])):
                if q < len(layouts) and layouts[q] == "nk":   # stored [n, K]
                    d.source[s].ptr = self.dev(np.asarray(x, f32).T).data_ptr()
                    d.source[s].stride_k, d.source[s].stride_i = 1, K
                else:
                    d.source[s].ptr = self.dev(x).data_ptr()
                    d.source[s].stride_k, d.source[s].stride_i = n, 1
                s += 1
            d.num_sources = s
            if f["family"] == "beta":
                d.draws = self.dev(f["draws"]).data_ptr()
                if f.get("dgrad") is not None:
                    d.dgrad = self.dev(f["dgrad"]).data_ptr()
                saved = self.nans((n, 4), torch.float64)
                if not f.get("no_saved"):
                    d.saved = saved.data_ptr()
            elif f.get("gen") is None:
                d.eps = self.dev(f["eps"]).data_ptr()
            else:
                g = f["gen"]
                d.seed, d.step, d.stream_id = g["seed"], g["step"], g["stream_id"]
                d.particle_offset, d.element_offset = g["particle_offset"], g["element_offset"]
                if g.get("step_device") is not None:
                    d.step_device = self.dev(np.asarray([g["step_device"]], np.int64)).data_ptr()
        self.saved.append(saved)

    def forward(self):
        code = self.lib.mi_elbo_forward(ctypes.byref(self.E), self.ws.data_ptr(), self.size,
                                        self.loss.data_ptr(), self.stream)
        torch.cuda.synchronize()
        return code

    def backward(self, u):
        for (grads, _) in self.grads:
            for g in grads:
                if g is not None:
                    g.fill_(NAN)
        for x, b in zip(self.buffers, self.case.get("buffers", [])):
            x.copy_(torch.as_tensor(b))
        self.dterm.fill_(NAN)
        up = torch.tensor(float(u), device=self.device)
        code = self.lib.mi_elbo_backward(ctypes.byref(self.E), up.data_ptr(), self.dterm.data_ptr(),
                                         self.ws.data_ptr(), self.size, self.stream)
        torch.cuda.synchronize()
        return code

    def grad(self, j):
        """[n, 2] with NaN for a NULL pointer; asserts the gaps of a strided gradient kept NaN."""
        grads, gs = self.grads[j]
        n = self.case["factors"][j]["n"]
        out = np.full((n, 2), np.nan)
        for q, g in enumerate(grads):
            if g is None:
                continue
            host = g.cpu().numpy()
            out[:, q] = host[::gs[q]][:n] if gs[q] else host[:1]
            if gs[q] > 1:
                gaps = np.ones(len(host), bool)
                gaps[::gs[q]] = False
                assert np.isnan(host[gaps]).all(), "a strided gradient's gaps were written"
        return out


def philox_normal(device, K, n, gen):
    """The generator's eps [K, n] for a factor's gen words, through mi_philox_normal."""
    width = gen["element_offset"] + n
    out = torch.empty((K, width), device=device)
    nat.check(nat.lib().mi_philox_normal(K, width, gen["seed"],
                                         gen["step"] + (gen.get("step_device") or 0),
                                         gen["stream_id"], gen["particle_offset"], out.data_ptr(),
                                         None), "mi_philox_normal")
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, gen["element_offset"]:]


def resolve(case, device):
    """Fill what the reference needs and the descriptor leaves to the launch: regenerated eps, and
    sources that are rows of the jobs' slot gradients (the reference's own, rounded to float)."""
    K = case["K"]
    jobs = [ref.reduce_job(job, K) for job in case.get("jobs", [])]
    for f in case.get("factors", []):
        if f.get("gen") is not None:
            f["eps"] = philox_normal(device, K, f["n"], f["gen"])
        if f.get("slot_sources"):
            rows = []
            for job, slot in f["slot_sources"]:
                sg = jobs[job]["slot_grad"].value.astype(f32)
                rows.append(sg[slot:slot + f["n"]].T if f["n"] > 1 else sg[slot][:, None])
            f["sources"] = rows + list(f.get("outside", []))
    return case


@pytest.fixture(scope="module")
def floor():
    return cases.device_floor()


def run_and_check(name, case, device, upstreams, floor=0.0, options=0, expect_final=False,
                  tails=(), **kw):
    """Forward (loss, reductions, saved sums, step words), then a backward per upstream. tails: the
    factors the forward finishes in the blocks that reduce their source rows, source by source in
    float64 (elbo_reference's `linear`): their `saved` sums and final gradients, and the backward
    of the Beta ones, which reads `saved`; a Normal one's backward sums the sources in float32."""
    resolve(case, device)
    L = Launch(case, device, options=options, **kw)
    assert L.size_code == 0
    nat.check(L.forward(), name)
    want = ref.elbo_reference(case, floor=floor, linear=tails)
    check(f"{name} loss", L.loss.item(), want["loss"])
    for j, (out, r) in enumerate(zip(L.jobs, want["jobs"])):
        if r["total"] is None:
            assert torch.isnan(out["total"]).all(), "a particle-summed job wrote totals"
        else:
            check(f"{name} job {j} total", out["total"].cpu().numpy(), r["total"])
        if out["site_lp"] is not None:
            check(f"{name} job {j} site_lp", out["site_lp"].cpu().numpy(), r["site_lp"],
                  rounding=False)
        if r["slot_grad"] is not None:
            check(f"{name} job {j} slot_grad", out["slot_grad"].cpu().numpy(), r["slot_grad"])
    for j, q in enumerate(want["saved"]):
        if q is not None:
            check(f"{name} factor {j} saved", L.saved[j].cpu().numpy(), q, "gradient",
                  rounding=False)
    if L.counter is not None:
        assert (L.snapshot.item(), L.counter.item()) == (41, 42)
    if L.mirror is not None:
        assert torch.equal(L.mirror, L.flags)
    if options & nat.ELBO_FINAL_GRADS:
        complete = ctypes.c_int(-1)
        nat.check(L.lib.mi_elbo_final_grads(ctypes.byref(L.E), ctypes.byref(complete)), name)
        assert bool(complete.value) == expect_final
        if complete.value:   # the forward alone left the gradients of an upstream of 1
            one = ref.elbo_reference(case, f32(1.0), floor=floor, linear=tails)
            for j, q in enumerate(one["grads"]):
                check(f"{name} factor {j} final gradient", L.grad(j), q, "gradient")
    for u in upstreams:
        nat.check(L.backward(u), name)
        want = ref.elbo_reference(case, f32(u), floor=floor, linear=[
            j for j in tails if case["factors"][j]["family"] == "beta"])
        check(f"{name} u={u} dterm", L.dterm.item(), want["dterm"])
        for j, q in enumerate(want["grads"]):
            got = L.grad(j)
            null = np.isnan(got).all(0) & np.asarray(case["factors"][j].get("storage", {}).get(
                "grad_null", (False, False)))
            assert null.tolist() == list(case["factors"][j].get("storage", {}).get(
                "grad_null", (False, False)))
            for p in range(2):
                if not null[p]:
                    col = ref.Q(q.value[:, p], {k: m[:, p] for k, m in q.mag.items()},
                                q.sum64[:, p], q.extra[:, p])
                    check(f"{name} u={u} factor {j} gradient {p}", got[:, p], col, "gradient")
        for b, (x, w) in enumerate(zip(L.buffers, want["buffers"])):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), w.view(np.uint32)), (name, u, b)
    if L.counter is not None:   # a second evaluation advances the words again
        nat.check(L.forward(), name)
        assert (L.snapshot.item(), L.counter.item()) == (42, 43)
    return L


# ---- case builders -----------------------------------------------------------------------------

def conc(n, shift=0):
    c = ref.CONCENTRATIONS
    return np.asarray([c[(i + shift) % len(c)] for i in range(n)], f32)


def rates(n, shift=0):
    return np.asarray([ref.RATES[(i + shift) % len(ref.RATES)] for i in range(n)], f32)


def normal(rng, n, transform=(0, 0), weight=1.0, **storage):
    scale = np.exp(rng.normal(size=n)).astype(f32)
    scale[:min(n, 4)] = rates(min(n, 4))
    return {"family": "normal", "n": n, "p0": rng.normal(size=n).astype(f32), "p1": scale,
            "weight": weight, "transform": transform, "draw": None, "storage": storage}


def gamma(n, transform=(0, 0), weight=1.0, shift=0, **storage):
    return {"family": "gamma", "n": n, "p0": conc(n, shift), "p1": rates(n, shift // 2),
            "weight": weight, "transform": transform, "draw": None, "storage": storage}


def beta(n, transform=(0, 0), weight=1.0, **storage):
    pairs = np.asarray([ref.BETA_PAIRS[i % len(ref.BETA_PAIRS)] for i in range(n)], f32)
    return {"family": "beta", "n": n, "p0": pairs[:, 0].copy(), "p1": pairs[:, 1].copy(),
            "weight": weight, "transform": transform, "draw": None, "storage": storage}


BUFFER_LENGTHS = (0, 1, 5000, 7, 300, 1024, 2, 0, 33, 4097, 5, 64, 255, 257, 1, 12)


def make_case(name, K, nterms, factors, es=1.0, nbuffers=0, jobs=()):
    rng = _rng(name)
    return {"K": K, "g0": f32(-1.0 / K), "entropy_scale": es,
            "terms": [rng.normal(size=K).astype(f32) for _ in range(nterms)],
            "factors": factors, "jobs": list(jobs),
            "buffers": [rng.normal(size=BUFFER_LENGTHS[b]).astype(f32) for b in range(nbuffers)]}


def entropy_cases():
    out = {}

    def add(name, K, nterms, factors, es=1.0, nbuffers=0):
        out[name] = lambda: make_case(name, K, nterms, factors(_rng(name + "f")), es, nbuffers)

    # Normal factors alone: the HAS_BETA = false kernel
    add("normal_n1_stride0", 1, 0, lambda r: [normal(r, 1, (0, 1), stride=(0, 0))])
    add("normal_n3", 3, 1, lambda r: [normal(r, 3, (1, 0), 0.25)], 1.0, 3)
    add("normal_n4", 256, 8, lambda r: [normal(r, 4, (1, 1))], 0.5, 16)
    add("normal_n5_grad_stride2", 3, 1, lambda r: [normal(r, 5, (0, 1), grad_stride=(2, 2))], 0.5)
    add("normal_n1023", 256, 0, lambda r: [normal(r, 1023, (0, 0), 0.25)], 0.5, 3)
    add("normal_n8191", 3, 1, lambda r: [normal(r, 8191, (0, 1))])
    add("normal_n8193", 1, 8, lambda r: [normal(r, 8193, (1, 1), 0.25)])
    add("normal_n70001", 256, 1, lambda r: [normal(r, 70001, (0, 0))], 0.5)
    add("normal_K8193", 8193, 8, lambda r: [normal(r, 5, (0, 0), grad_null=(True, False))])
    add("normal_unaligned", 3, 1, lambda r: [normal(r, 1023, (0, 1), offset=(0, 1))])
    add("normal_stride2", 3, 1, lambda r: [normal(r, 1023, (1, 1), stride=(2, 2))])
    # Gamma and Beta: the HAS_BETA = true kernel
    add("gamma_n1", 1, 0, lambda r: [gamma(1, (0, 0), shift=3)])
    add("gamma_n5_grad_null", 3, 1, lambda r: [gamma(5, (1, 0), 0.25, grad_null=(True, False))], 0.5)
    add("gamma_n257_grad_stride2", 256, 8, lambda r: [gamma(257, (1, 1), grad_stride=(2, 2))], 1.0, 3)
    add("gamma_every_rate", 3, 0, lambda r: [gamma(14, (0, 1), shift=0), gamma(14, (0, 0), shift=2),
                                             gamma(14, (1, 0), shift=4), gamma(14, (1, 1), shift=6)])
    add("beta_n1", 1, 1, lambda r: [beta(1, (1, 1))])
    add("beta_n5_grad_null", 3, 0, lambda r: [beta(5, (0, 1), 0.25, grad_null=(False, True))], 0.5)
    add("beta_n257_interleaved", 256, 1, lambda r: [beta(257, (1, 0), interleaved=True)], 1.0, 16)
    add("mixed_8_factors", 256, 8, lambda r: [
        normal(r, 1023, (1, 1), 0.25), gamma(5, (0, 1)), beta(257, (0, 0), 0.25, interleaved=True),
        normal(r, 4, (0, 0)), gamma(257, (1, 0), 0.25, shift=5), beta(1, (1, 1)),
        normal(r, 5, (0, 1), 0.25, stride=(2, 2)), beta(5, (0, 1), grad_stride=(2, 2))], 0.5, 3)
    return out


ENTROPY = entropy_cases()


@pytest.mark.parametrize("name", sorted(ENTROPY))
def test_terms_and_entropy(device, name):
    """a. draw_kind NONE: the loss, dterm, every entropy gradient at u = 1, 2.5 and -0.5 with both
    transforms, NULL and strided gradients, the buffers, the step words and the flag mirror."""
    run_and_check(name, ENTROPY[name](), device, (1.0, 2.5, -0.5), counters=True, nflags=300)


def with_sources(rng, f, K, count, zero_rows=(), layouts=()):
    src = [rng.normal(size=(K, f["n"])).astype(f32) for _ in range(count)]
    for s in src:
        s[list(zero_rows)] = 0.0
    f.update(draw="sources", sources=src, source_layout=list(layouts))
    return f


def absorbed_cases():
    out = {}
    for q, (n, K) in enumerate(ref.NORMAL_SOURCES):
        def build(n=n, K=K, q=q):
            rng = _rng(f"ns{n}_{K}")
            f = with_sources(rng, normal(rng, n, ((0, 1), (1, 1))[q % 2], (1.0, 0.25)[q % 2]), K,
                             (1, 4)[q % 2], layouts=("kn", "nk"))
            f["eps"] = rng.normal(size=(K, n)).astype(f32)
            return make_case(f"ns{n}_{K}", K, 1, [f, gamma(5)], (1.0, 0.5)[q % 2])
        out[f"normal_sources_n{n}_K{K}"] = build
    for off in (0, 8):
        def build(off=off):
            rng = _rng(f"regen{off}")
            f = with_sources(rng, normal(rng, 300, (0, 1)), 8, 4, layouts=("nk",))
            f["gen"] = {"seed": 1234, "step": 3, "stream_id": 7, "particle_offset": 2,
                        "element_offset": off, "step_device": 5}
            return make_case(f"regen{off}", 8, 0, [f])
        out[f"normal_regenerated_offset{off}"] = build
    for rows, n, gs in ref.PARTIALS:
        def build(rows=rows, n=n, gs=gs):
            rng = _rng(f"p{rows}_{n}_{gs}")
            f = normal(rng, n, ((0, 1), (1, 1))[n % 2], 0.25, grad_stride=(gs, gs))
            f.update(draw="partials", partial=[rng.normal(size=(rows, n)).astype(f32) for _ in "ab"])
            return make_case(f"p{rows}_{n}_{gs}", 8, 1, [f], 0.5)
        out[f"partials_rows{rows}_n{n}_gs{gs}"] = build
    for n, K in ref.BETA_DGRAD:
        def build(n=n, K=K):
            rng = _rng(f"bd{n}_{K}")
            f = with_sources(rng, beta(n, ((1, 1), (0, 1))[n % 2], 0.25, interleaved=True), K,
                             (1, 4)[K % 2], zero_rows=(0, K // 2), layouts=("kn", "nk"))
            f.update(draws=rng.uniform(0.01, 0.99, (K, n)).astype(f32), dgrad=rng.normal(size=(K, n, 2)))
            return make_case(f"bd{n}_{K}", K, 1, [f, normal(rng, 5)], 0.5)
        out[f"beta_dgrad_n{n}_K{K}"] = build

    def inline():
        x, c1, c0 = cases.beta_grid()
        K, n = x.shape
        rng = _rng("inline")
        f = with_sources(rng, beta(n, (1, 0)), K, 2, zero_rows=(1, K - 1))
        f.update(p0=c1, p1=c0, draws=x, dgrad=None)
        return make_case("inline", K, 1, [f])
    out["beta_inline_every_regime"] = inline
    return out


ABSORBED = absorbed_cases()


@pytest.mark.parametrize("name", sorted(ABSORBED))
def test_absorbed_draws(device, name, floor):
    """b. Absorbed draws without reductions, after forward + backward at u = 1 and 2.5: every
    reducing path of add_absorbed, and `saved` of the forward-absorbed Beta factors."""
    case = ABSORBED[name]()
    x = case["factors"][0].get("draws")
    assert x is None or ((x > 0) & (x < 1)).all()
    # (a launch of fused-draw factors alone also finishes them in the forward: MI_ELBO_FINAL_GRADS)
    fused = name.startswith("partials")
    run_and_check(name, case, device, (1.0, 2.5), floor=floor,
                  options=nat.ELBO_FINAL_GRADS if fused else 0, expect_final=fused)


def job(rng, nseg, K, ns, nl, rank1=(), ksum=0, site_lp=False):
    values = []
    for v in range((0 if ksum else ns) + nl):
        if v in rank1:
            values.append({"u": rng.normal(size=nseg).astype(f32), "f": rng.normal(size=K).astype(f32),
                           "e": rng.normal(size=K).astype(f32)})
        else:
            values.append(rng.normal(size=(nseg, K)).astype(f32))
    return {"nseg": nseg, "num_sites": ns, "num_slots": nl, "scale": [1.0, -0.375][:ns],
            "slot_scale": 0.75, "values": values, "site_lp": site_lp,
            "ksum": rng.normal(size=(ns, ksum)) if ksum else None}


def tail_beta(rng, K, slot_sources):
    """A one-element forward-absorbed Beta factor fed by a slot row and an outside array."""
    f = beta(1, (1, 0), 0.25, interleaved=True)
    f.update(p0=np.asarray([2.5], f32), p1=np.asarray([0.3], f32), draw="sources",
             slot_sources=slot_sources, outside=[rng.normal(size=(K, 1)).astype(f32)],
             draws=rng.uniform(0.01, 0.99, (K, 1)).astype(f32), dgrad=rng.normal(size=(K, 1, 2)))
    return f


def tail_normal(rng, n, slot_sources):
    f = normal(rng, n, (0, 1))
    f.update(draw="sources", slot_sources=slot_sources, source_layout=[],
             gen={"seed": 99, "step": 11, "stream_id": 2, "particle_offset": 1, "element_offset": 4})
    return f


def reduce_cases():
    out = {}

    def add(name, K, nterms, jobs, factors=lambda r: [], final=False):
        def build():
            rng = _rng(name)
            return make_case(name, K, nterms, factors(rng), 0.5, 0, jobs(rng))
        out[name] = (build, final)

    add("nseg1", 100, 1, lambda r: [job(r, 1, 100, 1, 0)])
    add("nseg2_two_sites_site_lp", 100, 0, lambda r: [job(r, 2, 100, 2, 2, site_lp=True)])
    add("nseg70_rank1", 100, 1, lambda r: [job(r, 70, 100, 1, 2, rank1=(1,))])
    add("nseg520_two_sites", 100, 0, lambda r: [job(r, 520, 100, 2, 0)])
    add("nseg800", 100, 0, lambda r: [job(r, 800, 100, 1, 2)])
    add("nseg70_K4096", 4096, 1, lambda r: [job(r, 70, 4096, 1, 1)])
    add("ksum_and_plain", 100, 1, lambda r: [job(r, 2, 100, 2, 2, ksum=37), job(r, 70, 100, 1, 0)])
    # tails: factor 0 a one-element Normal fed from slots of both jobs, factor 1 a Beta tail
    add("tails_single", 100, 0, lambda r: [job(r, 70, 100, 1, 2), job(r, 2, 100, 2, 1)],
        lambda r: [tail_normal(r, 1, [(0, 0), (0, 1), (1, 0)]), tail_beta(r, 100, [(0, 1)])], True)
    # factor 0 a three-element Normal over consecutive slot rows (stride_i = K) of a split job
    add("tails_rows", 100, 1, lambda r: [job(r, 2, 100, 1, 4)],
        lambda r: [tail_normal(r, 3, [(0, 1)]), tail_beta(r, 100, [(0, 0)])], True)
    return out


REDUCE = reduce_cases()


@pytest.mark.parametrize("external", [False, True])
@pytest.mark.parametrize("name", sorted(REDUCE))
def test_deferred_reductions(device, monkeypatch, name, external):
    """c. total, site_lp, slot_grad and the loss of every kred variant, a rank-one value and a
    particle-summed job; tails fed from the slots; the same as launches of their own
    (MININF_AMD_ELBO_EXTERNAL=1); and with MI_ELBO_FINAL_GRADS the gradients the forward leaves."""
    if external:
        monkeypatch.setenv("MININF_AMD_ELBO_EXTERNAL", "1")
    else:
        monkeypatch.delenv("MININF_AMD_ELBO_EXTERNAL", raising=False)
    build, final = REDUCE[name]
    # (in the launch, the two tail factors' sources enter source by source; with the reductions as
    # launches of their own the lead blocks sum each particle's sources in float32 first)
    run_and_check(name, build(), device, (2.5,) if final else (1.0, 2.5),
                  options=nat.ELBO_FINAL_GRADS if final else 0, expect_final=final and not external,
                  tails=(0, 1) if final and not external else ())


# ---- d. argument checks: nothing is launched ------------------------------------------------------

def _untouched(L):
    outs = [L.loss.reshape(1), L.dterm] + [g for grads, _ in L.grads for g in grads if g is not None]
    outs += [s for s in L.saved if s is not None]
    for out in L.jobs:
        outs += [v for v in out.values() if v is not None]
    return all(bool(torch.isnan(o).all()) for o in outs)


def _refused(L, code, forward_only=False):
    assert L.forward() == code
    if not forward_only:
        assert L.backward(1.0) == code
    assert _untouched(L)


def test_argument_checks_launch_nothing(device):
    rng = _rng("args")

    def simple(factors, jobs=()):
        return resolve(make_case("args", 8, 1, factors, 1.0, 0, jobs), device)

    L = Launch(simple([normal(rng, 5)]), device)
    L.E.factors[0].weight = 0.0
    _refused(L, nat.MI_EINVAL)
    f = with_sources(rng, normal(rng, 5), 8, 1)
    f["gen"] = {"seed": 1, "step": 0, "stream_id": 0, "particle_offset": 0, "element_offset": 2}
    _refused(Launch(make_case("args", 8, 1, [f]), device), nat.MI_EINVAL)
    g = with_sources(rng, gamma(5), 8, 1)
    g["eps"] = np.zeros((8, 5), f32)
    _refused(Launch(simple([g]), device), nat.MI_EINVAL)
    L = Launch(simple([normal(rng, 5) for _ in range(8)]), device)
    L.E.num_factors = 9
    _refused(L, nat.MI_EINVAL)
    b = with_sources(rng, beta(3), 8, 1)
    b.update(draws=rng.uniform(0.1, 0.9, (8, 3)).astype(f32), dgrad=rng.normal(size=(8, 3, 2)),
             no_saved=True)
    _refused(Launch(simple([b]), device), nat.MI_EINVAL)
    b = with_sources(rng, beta(3), 8, 1)
    b.update(draws=rng.uniform(0.1, 0.9, (8, 3)).astype(f32), dgrad=None)
    _refused(Launch(simple([b], [job(rng, 2, 8, 1, 0)]), device), nat.MI_EUNSUPPORTED,
             forward_only=True)
    L = Launch(simple([normal(rng, 5)]), device)
    L.size -= 1
    _refused(L, nat.MI_EWORKSPACE)
