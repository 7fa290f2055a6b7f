"""
The plumbing between ``guide.draw`` / ``guide.entropy`` and the native entry points, for each of
the twelve native guide families on the MI355X: the draw against a direct call of the family's
``mi_*_rsample`` with the same Philox key, the parameter gradients of ``(draw * w).sum()`` against
a direct call of ``mi_*_rsample_backward``, and the entropy and its gradients under an upstream of
0.5 against a direct call of ``mi_*_entropy``. Both sides run the same kernel on the same inputs,
so everything is compared with ``torch.equal``. The key is spelled here from literals, every
argument distinct (particle offset 2, stream id 1, a non-zero device step word, and a forward word
that has moved on before the backward runs), so that no two of its arguments can be swapped.
"""
import ctypes

import pytest
import torch
from torch.distributions import Beta, Cauchy, Dirichlet, Exponential, Gamma, HalfCauchy, \
    HalfNormal, Laplace, LogNormal, LowRankMultivariateNormal, MultivariateNormal, Normal

from mininf_amd import _native as nat, guide

pytestmark = pytest.mark.gpu

K, N, D, R, C = 3, 5, 3, 2, 3
SEED, STEP, STREAM, OFFSET, WORD, ELEMENT = 0x9E3779B97F4A7C15, 7, 1, 2, 5, 4
LAYOUTS = ("dense", "scalar", "strided")


def key(word, noise, element=None):
    """seed, step, step word, stream id, particle offset, [element offset,] noise: the ABI order."""
    if element is None:
        return SEED, STEP, word.data_ptr(), STREAM, OFFSET, nat.ptr(noise)
    return SEED, STEP, word.data_ptr(), STREAM, OFFSET, element, nat.ptr(noise)


def workspace(device, query, *dims):
    size = ctypes.c_size_t()
    nat.check(getattr(nat.lib(), query)(*dims, ctypes.byref(size)), query)
    return torch.empty(max(1, size.value), dtype=torch.uint8, device=device), size.value


def call(name, *args):
    nat.check(getattr(nat.lib(), name)(*args, None), name)


def filled(device, *shape):
    return torch.full(shape, float("nan"), device=device)


class Param:
    """A leaf and the view of it a factor is given: the leaf itself ("dense": [n]; "scalar": 0-d,
    read with stride 0), or every second element of it ("strided": what _flat_param copies)."""
    def __init__(self, values, layout, device):
        values = torch.as_tensor(values, dtype=torch.float32)
        if layout == "strided":
            self.leaf = torch.zeros(2 * values.numel()).to(device)
            self.leaf[::2] = values.to(device)
            self.leaf.requires_grad_()
            self.view = self.leaf[::2]
        else:
            self.leaf = values.to(device).requires_grad_()
            self.view = self.leaf
        self.flat = self.view.detach().reshape(-1).contiguous()
        self.stride = 0 if self.flat.numel() == 1 else 1

    def grad(self):
        grad = self.leaf.grad[::2] if self.view is not self.leaf else self.leaf.grad
        return grad.reshape(-1)


def values(n, generator, low=0.5, high=1.5):
    return low + (high - low) * torch.rand(n, generator=generator)


class Words:
    """The forward's device step word and the snapshot its backward reads, both WORD."""
    def __init__(self, device):
        self.forward = torch.full((1,), WORD, dtype=torch.int64, device=device)
        self.snapshot = torch.full((1,), WORD, dtype=torch.int64, device=device)

    def config(self, noise, element=0):
        return guide.DrawConfig(K=K, seed=SEED, step=STEP, stream_id=STREAM,
                                particle_offset=OFFSET, noise=noise, step_device=self.forward,
                                step_snapshot=self.snapshot, element_offset=element)

    def advance(self):
        """As the ELBO forward does between a draw and its backward."""
        self.forward.add_(1)


def backward(draw, generator):
    """d (draw * w).sum(): returns the upstream w, [K, n] as the backward kernels get it."""
    w = torch.randn(draw.shape, generator=generator).to(draw.device)
    (draw * w).sum().backward()
    return w.reshape(K, -1)


# ---- Normal, Gamma and the one-noise-word families: [N] parameters with strides ----------------
# name -> (class, MI_PRED_* code or None, parameters (a, b) in the entry point's order, base noise)
FLAT = {
    "normal": (Normal, None, ("loc", "scale"), "normal"),
    "gamma": (Gamma, None, ("concentration", "rate"), "positive"),
    "exponential": (Exponential, nat.PRED_EXPONENTIAL, ("rate",), "uniform"),
    "laplace": (Laplace, nat.PRED_LAPLACE, ("loc", "scale"), "uniform"),
    "cauchy": (Cauchy, nat.PRED_CAUCHY, ("loc", "scale"), "uniform"),
    "half_cauchy": (HalfCauchy, nat.PRED_HALF_CAUCHY, ("scale",), "uniform"),
    "half_normal": (HalfNormal, nat.PRED_HALF_NORMAL, ("scale",), "normal"),
    "log_normal": (LogNormal, nat.PRED_LOG_NORMAL, ("loc", "scale"), "normal"),
}


def base_noise(kind, generator, device, *shape):
    if kind == "normal":
        noise = torch.randn(shape, generator=generator)
    else:   # uniforms inside (0, 1); standard Gamma draws and Beta draws likewise
        noise = 0.05 + 0.9 * torch.rand(shape, generator=generator)
    return noise.to(device)


@pytest.mark.parametrize("injected", (False, True), ids=("philox", "injected"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(FLAT))
def test_flat_family_draw_and_gradients(device, name, layout, injected):
    cls, code, names, kind = FLAT[name]
    generator = torch.Generator().manual_seed(len(name) + 10 * LAYOUTS.index(layout))
    n = 1 if layout == "scalar" else N
    # the first parameter takes the layout; with "strided" the others stay dense
    params = [Param(values(n, generator) if layout != "scalar" else values(1, generator)[0],
                    layout if i == 0 else layout.replace("strided", "dense"), device)
              for i in range(len(names))]
    factor = cls(**{field: p.view for field, p in zip(names, params)}, validate_args=False)
    noise = base_noise(kind, generator, device, K, n) if injected else None
    words = Words(device)
    element = ELEMENT if name == "normal" else 0
    draw = guide.draw(factor, words.config(noise, element))
    assert draw.shape == (K,) + tuple(factor.batch_shape)

    a, b = params[0], params[1] if len(params) > 1 else None
    pointers = (a.flat.data_ptr(), a.stride, None if b is None else b.flat.data_ptr(),
                0 if b is None else b.stride)
    want, g = filled(device, K, n), filled(device, K, n)
    if name == "normal":
        call("mi_normal_rsample", *pointers, K, n, *key(words.forward, noise, ELEMENT),
             want.data_ptr())
    elif name == "gamma":
        call("mi_gamma_rsample", *pointers, K, n, *key(words.forward, noise), g.data_ptr(),
             want.data_ptr())
    else:
        call("mi_elementwise_rsample", code, *pointers, K, n, *key(words.forward, noise),
             want.data_ptr())
    assert torch.isfinite(want).all()
    assert torch.equal(draw.reshape(K, n), want)

    words.advance()
    dz = backward(draw, generator)
    da = filled(device, n)
    db = filled(device, n) if b is not None else None
    upstream = (dz.data_ptr(), dz.stride(0), dz.stride(1))
    if name == "normal":
        ws, size = workspace(device, "mi_normal_rsample_backward_workspace_bytes", K, n)
        call("mi_normal_rsample_backward", *upstream, K, n,
             *key(words.snapshot, noise, ELEMENT), ws.data_ptr(), size, da.data_ptr(),
             db.data_ptr())
    elif name == "gamma":
        ws, size = workspace(device, "mi_gamma_rsample_backward_workspace_bytes", K, n)
        call("mi_gamma_rsample_backward", *upstream, g.data_ptr(), *pointers, K, n,
             ws.data_ptr(), size, da.data_ptr(), 1, db.data_ptr(), 1)
    else:
        ws, size = workspace(device, "mi_elementwise_rsample_backward_workspace_bytes", K, n)
        call("mi_elementwise_rsample_backward", code, *upstream, *pointers, K, n,
             *key(words.snapshot, noise), ws.data_ptr(), size, da.data_ptr(), nat.ptr(db))
    assert torch.equal(a.grad(), da)
    if b is not None:
        assert torch.equal(b.grad(), db)


# ---- Beta: the interleaved [N, 2] concentrations -----------------------------------------------
@pytest.mark.parametrize("injected", (False, True), ids=("philox", "injected"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_beta_draw_and_gradients(device, layout, injected):
    generator = torch.Generator().manual_seed(20 + LAYOUTS.index(layout))
    n = 1 if layout == "scalar" else N
    c1 = Param(values(n, generator) if n > 1 else values(1, generator)[0], layout, device)
    c0 = Param(values(n, generator) if n > 1 else values(1, generator)[0],
               layout.replace("strided", "dense"), device)
    factor = Beta(c1.view, c0.view, validate_args=False)
    noise = base_noise("uniform", generator, device, K, n) if injected else None   # the draws
    words = Words(device)
    draw = guide.draw(factor, words.config(noise))
    conc = torch.stack([c1.flat, c0.flat], -1).contiguous()
    base = conc.data_ptr()
    want = filled(device, K, n)
    call("mi_beta_rsample", base, 2, base + 4, 2, K, n, *key(words.forward, noise),
         want.data_ptr())
    assert torch.isfinite(want).all()
    assert torch.equal(draw.reshape(K, n), want)

    words.advance()
    dx = backward(draw, generator)
    ws, size = workspace(device, "mi_beta_rsample_backward_workspace_bytes", K, n)
    dconc = filled(device, n, 2)
    out = dconc.data_ptr()
    call("mi_beta_rsample_backward", dx.data_ptr(), dx.stride(0), dx.stride(1), want.data_ptr(),
         base, 2, base + 4, 2, K, n, ws.data_ptr(), size, out, 2, out + 4, 2)
    assert torch.equal(c1.grad(), dconc[:, 0])
    assert torch.equal(c0.grad(), dconc[:, 1])


# ---- MultivariateNormal, LowRankMultivariateNormal, Dirichlet ----------------------------------
@pytest.mark.parametrize("injected", (False, True), ids=("philox", "injected"))
def test_mvn_draw_and_gradients(device, injected):
    generator = torch.Generator().manual_seed(30)
    loc = torch.randn(D, generator=generator).to(device).requires_grad_()
    tril = (torch.randn(D, D, generator=generator).tril(-1) +
            torch.diag(values(D, generator))).to(device).requires_grad_()
    noise = base_noise("normal", generator, device, K, D) if injected else None
    words = Words(device)
    draw = guide.draw(MultivariateNormal(loc, scale_tril=tril, validate_args=False),
                      words.config(noise))
    want = filled(device, K, D)
    call("mi_mvn_rsample", loc.data_ptr(), tril.data_ptr(), K, D, *key(words.forward, noise),
         want.data_ptr())
    assert torch.isfinite(want).all()
    assert torch.equal(draw, want)

    words.advance()
    dz = backward(draw, generator)
    ws, size = workspace(device, "mi_mvn_rsample_backward_workspace_bytes", K, D)
    dloc, dtril = filled(device, D), filled(device, D, D)
    call("mi_mvn_rsample_backward", dz.data_ptr(), dz.stride(0), dz.stride(1), K, D,
         *key(words.snapshot, noise), ws.data_ptr(), size, dloc.data_ptr(), dtril.data_ptr())
    assert torch.equal(loc.grad, dloc)
    assert torch.equal(tril.grad, dtril)


def lowrank_factor(device, generator):
    loc = torch.randn(D, generator=generator).to(device).requires_grad_()
    cov_factor = (0.3 * torch.randn(D, R, generator=generator)).to(device).requires_grad_()
    cov_diag = values(D, generator).to(device).requires_grad_()
    return loc, cov_factor, cov_diag, LowRankMultivariateNormal(loc, cov_factor, cov_diag,
                                                                validate_args=False)


@pytest.mark.parametrize("injected", (False, True), ids=("philox", "injected"))
def test_lowrank_draw_and_gradients(device, injected):
    generator = torch.Generator().manual_seed(40)
    loc, cov_factor, cov_diag, factor = lowrank_factor(device, generator)
    noise = base_noise("normal", generator, device, K, D + R) if injected else None
    words = Words(device)
    draw = guide.draw(factor, words.config(noise))
    want = filled(device, K, D)
    call("mi_lowrank_rsample", loc.data_ptr(), cov_factor.data_ptr(), cov_diag.data_ptr(), K, D, R,
         *key(words.forward, noise), want.data_ptr())
    assert torch.isfinite(want).all()
    assert torch.equal(draw, want)

    words.advance()
    dz = backward(draw, generator)
    ws, size = workspace(device, "mi_lowrank_rsample_backward_workspace_bytes", K, D, R)
    dloc, dfactor, ddiag = filled(device, D), filled(device, D, R), filled(device, D)
    call("mi_lowrank_rsample_backward", dz.data_ptr(), dz.stride(0), dz.stride(1),
         cov_diag.data_ptr(), K, D, R, *key(words.snapshot, noise), ws.data_ptr(), size,
         dloc.data_ptr(), dfactor.data_ptr(), ddiag.data_ptr())
    # (the constructor's capacitance graph hangs on the same leaves: the draw alone is in here)
    assert torch.equal(loc.grad, dloc)
    assert torch.equal(cov_factor.grad, dfactor)
    assert torch.equal(cov_diag.grad, ddiag)


def dirichlet_leaf(device, generator, layout):
    """(leaf, the concentration a factor gets, its gradient's view): [N, C]; [C], unbatched; or
    every second row of a [2 N, C] leaf."""
    if layout == "scalar":
        leaf = values(C, generator).to(device).requires_grad_()
        return leaf, leaf, lambda: leaf.grad.reshape(1, C)
    if layout == "dense":
        leaf = values(N * C, generator).reshape(N, C).to(device).requires_grad_()
        return leaf, leaf, lambda: leaf.grad
    leaf = values(2 * N * C, generator).reshape(2 * N, C).to(device).requires_grad_()
    return leaf, leaf[::2], lambda: leaf.grad[::2]


@pytest.mark.parametrize("injected", (False, True), ids=("philox", "injected"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dirichlet_draw_and_gradients(device, layout, injected):
    generator = torch.Generator().manual_seed(50 + LAYOUTS.index(layout))
    leaf, view, grad = dirichlet_leaf(device, generator, layout)
    n = 1 if layout == "scalar" else N
    factor = Dirichlet(view, validate_args=False)
    noise = base_noise("positive", generator, device, K, n, C) if injected else None
    words = Words(device)
    draw = guide.draw(factor, words.config(noise))
    assert draw.shape == (K,) + tuple(factor.batch_shape) + (C,)
    conc = view.detach().reshape(n, C).contiguous()
    want = filled(device, K, n, C)
    call("mi_dirichlet_rsample", conc.data_ptr(), K, n, C, *key(words.forward, noise),
         want.data_ptr())
    assert torch.isfinite(want).all()
    assert torch.equal(draw.reshape(K, n, C), want)

    words.advance()
    dx = backward(draw, generator).reshape(K, n, C)
    ws, size = workspace(device, "mi_dirichlet_rsample_backward_workspace_bytes", K, n, C)
    dconc = filled(device, n, C)
    call("mi_dirichlet_rsample_backward", dx.data_ptr(), *dx.stride(), want.data_ptr(),
         conc.data_ptr(), K, n, C, ws.data_ptr(), size, dconc.data_ptr())
    assert torch.equal(grad(), dconc)


# ---- the entropies -----------------------------------------------------------------------------
HALF = 0.5


def test_dirichlet_entropy_and_gradient(device):
    generator = torch.Generator().manual_seed(60)
    leaf, view, grad = dirichlet_leaf(device, generator, "dense")
    h = guide.entropy(Dirichlet(view, validate_args=False))
    h.backward(torch.tensor(HALF, device=device))
    want, dconc = filled(device), filled(device, N, C)
    call("mi_dirichlet_entropy", leaf.data_ptr(), N, C, want.data_ptr(), dconc.data_ptr())
    assert torch.isfinite(want)
    assert torch.equal(h.detach(), want)
    assert torch.equal(grad(), dconc * torch.tensor(HALF, device=device))


def test_lowrank_entropy_and_gradient(device):
    generator = torch.Generator().manual_seed(61)
    loc, cov_factor, cov_diag, factor = lowrank_factor(device, generator)
    guide.draw_all({}, K, seed=SEED, step=STEP, particle_offset=OFFSET)
    h = guide.entropy(factor)
    assert guide.counts()["lowrank_entropies"] == 1
    h.backward(torch.tensor(HALF, device=device))
    tril = factor._capacitance_tril.detach().contiguous()
    ws, size = workspace(device, "mi_lowrank_entropy_workspace_bytes", D, R)
    want, dfactor, ddiag = filled(device), filled(device, D, R), filled(device, D)
    call("mi_lowrank_entropy", cov_factor.data_ptr(), cov_diag.data_ptr(), tril.data_ptr(), D, R,
         ws.data_ptr(), size, want.data_ptr(), dfactor.data_ptr(), ddiag.data_ptr())
    assert torch.isfinite(want)
    assert torch.equal(h.detach(), want)
    half = torch.tensor(HALF, device=device)
    assert loc.grad is None
    assert torch.equal(cov_factor.grad, dfactor * half)
    assert torch.equal(cov_diag.grad, ddiag * half)


@pytest.mark.parametrize("name", [name for name, spec in FLAT.items() if spec[1] is not None])
def test_elementwise_entropy_and_gradient(device, name):
    cls, code, names, _ = FLAT[name]
    generator = torch.Generator().manual_seed(70 + len(name))
    params = [Param(values(N, generator), "dense", device) for _ in names]
    h = guide.entropy(cls(**{field: p.view for field, p in zip(names, params)},
                          validate_args=False))
    h.backward(torch.tensor(HALF, device=device))
    a, b = params[0], params[1] if len(params) > 1 else None
    # (the entropy of a Laplace or Cauchy factor does not depend on its loc: no gradient asked)
    no_da = name in ("laplace", "cauchy")
    want, da = filled(device), None if no_da else filled(device, N)
    db = filled(device, N) if b is not None else None
    call("mi_elementwise_entropy", code, a.flat.data_ptr(), 1, None if b is None else
         b.flat.data_ptr(), 0 if b is None else 1, N, want.data_ptr(), nat.ptr(da), nat.ptr(db))
    assert torch.isfinite(want)
    assert torch.equal(h.detach(), want)
    half = torch.tensor(HALF, device=device)
    if no_da:
        assert a.leaf.grad is None
    else:
        assert torch.equal(a.grad(), da * half)
    if b is not None:
        assert torch.equal(b.grad(), db * half)


# ---- the counters ------------------------------------------------------------------------------
def test_counts_after_one_factor_of_every_family(device):
    generator = torch.Generator().manual_seed(80)
    one = torch.ones(N, device=device)
    _, _, _, lowrank = lowrank_factor(device, generator)
    factors = {
        "normal": Normal(0 * one, one), "beta": Beta(2 * one, one), "gamma": Gamma(2 * one, one),
        "mvn": MultivariateNormal(torch.zeros(D, device=device),
                                  scale_tril=torch.eye(D, device=device)),
        "dirichlet": Dirichlet(torch.ones(N, C, device=device)), "lowrank": lowrank,
        "elementwise": LogNormal(0 * one, one),
    }
    draws = guide.draw_all(factors, K, seed=SEED, step=STEP, particle_offset=OFFSET)
    assert guide.counts() == {"mvn_draws": 1, "dirichlet_draws": 1, "lowrank_draws": 1,
                              "elementwise_draws": 1, "lowrank_entropies": 0}
    for name, factor in factors.items():
        assert draws[name].shape == (K,) + tuple(factor.batch_shape) + tuple(factor.event_shape)
        assert torch.isfinite(draws[name]).all(), name
    guide.draw_all({}, K, seed=SEED, step=STEP, particle_offset=OFFSET)
    assert not any(guide.counts().values())
