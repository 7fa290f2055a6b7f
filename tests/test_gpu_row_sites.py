"""
The row sites' one autograd function (``engine._rows._RowSiteFn``) on the GPU, for each of the
seven kinds: Categorical, Dirichlet (its value a latent that requires grad), Normal mixture,
Categorical on ``X @ Theta``, and the gathered Normal site plain, ``+ X @ theta`` and with one
slope. Shapes K = 3, N = 5, C = 3, P = 2, G = 2 (group 1 holds a single row); each kind without and
with a mask (a MaskedTensor observation: the masked Dirichlet site's value is therefore observed),
and, where a kind has more than one parameter, once with one of them not requiring grad.

Through ``engine.log_joint`` (no prior sites: the parameters are sampled under ``no_log_prob``, so
the log joint is the row site alone), a non-unit per-particle upstream ``u`` is backpropagated
into every parameter and compared with float64 torch autograd of the model as written. Per kind:

* every parameter that requires grad receives a gradient of its own shape, within the bound the
  family's own GPU test file sets for its gradients:
  Categorical   rtol 1e-5, atol 1e-5 of the gradient's max-norm (test_gpu_kernels.py,
                test_categorical_model_against_oracle);
  Dirichlet     rtol 2e-5, atol 2e-5 (test_gpu_dirichlet.py, GRAD_RTOL / GRAD_ATOL);
  mixture       2e-5 of the gradient's max-norm (test_gpu_mixture.py, test_loss_against_float64);
  softmax       |error| <= 1e-5 |g0| bound + 1e-7 (test_gpu_softmax_linear.py, fractions) and
  gathered      the same (test_gpu_gather_site.py, test_gpu_gather_linear_site.py,
                test_gpu_gather_slopes_site.py), with ``bound`` the sum over the rows of the
                absolute terms of the gradient, as those files' references define it, and the
                upstream |u_k| where those launches have |g0|;
* a parameter that does not require grad receives None and the backward rescales nothing for it
  (one ``_scale_rows`` call per gradient wanted);
* ``holder["flags"]`` is one zero word.
"""
import numpy as np
import pytest
import torch
from torch.distributions import (Categorical, Dirichlet, Gamma, LogNormal, MixtureSameFamily,
                                 Normal)

import mininf_amd as mi
from mininf_amd import engine, particles
from mininf_amd.engine import _rows

pytestmark = pytest.mark.gpu

K, N, C, P, G = 3, 5, 3, 2, 2
U = (0.5, -2.0, 3.0)
GROUP = (0, 1, 0, 0, 0)
MASK = (True, True, False, True, True)

# kind: (the parameters' shapes, those drawn positive, the launcher's (linear, slopes) or None)
KINDS = {
    "categorical": ({"theta": (C,)}, (), None),
    "dirichlet": ({"conc": (N, C), "x": (N, C)}, ("conc",), None),
    "dirichlet_observed": ({"conc": (N, C)}, ("conc",), None),
    "mixture": ({"w": (C,), "mu": (C,), "sd": (C,)}, ("w", "sd"), None),
    "softmax": ({"theta": (P, C)}, (), ()),
    "gather": ({"alpha": (G,), "sigma": ()}, ("sigma",), (False, False)),
    "gather_linear": ({"alpha": (G,), "theta": (P,), "sigma": ()}, ("sigma",), (True, False)),
    "gather_slope": ({"alpha": (G,), "beta": (G,), "sigma": ()}, ("sigma",), (False, True)),
}

# (kind, masked, the parameter that does not require grad)
CASES = [
    ("categorical", False, None), ("categorical", True, None),
    ("dirichlet", False, None), ("dirichlet", False, "conc"), ("dirichlet_observed", True, None),
    ("mixture", False, None), ("mixture", True, "mu"),
    ("softmax", False, None), ("softmax", True, None),
    ("gather", False, None), ("gather", True, "sigma"),
    ("gather_linear", False, None), ("gather_linear", True, "theta"),
    ("gather_slope", False, None), ("gather_slope", True, "beta"),
]


def inputs(kind):
    """(the parameters [K, ...] float32, the data) of a kind, on the host."""
    rng = np.random.default_rng(sorted(KINDS).index(kind) + 5)
    shapes, positive, _ = KINDS[kind]
    params = {}
    for name, shape in shapes.items():
        draw = rng.normal(size=(K,) + shape)
        params[name] = torch.as_tensor((np.exp(0.4 * draw) if name in positive else draw)
                                       .astype(np.float32))
    for name in ("w", "x"):   # on the simplex
        if name in params:
            rows = torch.as_tensor(rng.dirichlet(np.full(C, 2.0), size=params[name].shape[:-1]))
            params[name] = rows.float()
    data = {"X": torch.as_tensor(rng.normal(size=(N, P)).astype(np.float32)),
            "z": torch.as_tensor(rng.normal(size=N).astype(np.float32)),
            "labels": torch.as_tensor(rng.integers(0, C, N)),
            "y": torch.as_tensor(rng.normal(size=N).astype(np.float32)),
            "rows": torch.as_tensor(rng.dirichlet(np.full(C, 2.0), size=N).astype(np.float32)),
            "group": torch.as_tensor(GROUP)}
    return params, data


def make_model(kind, d):
    """The model as written; ``d``: the data on the device."""
    def parameter(name, prior=Normal(0, 1)):
        with mi.no_log_prob():
            return mi.sample(name, prior, sample_shape=KINDS[kind][0][name])

    def model():
        if kind == "categorical":
            mi.sample("y", Categorical(logits=parameter("theta")), sample_shape=[N])
        elif kind in ("dirichlet", "dirichlet_observed"):
            mi.sample("x", Dirichlet(parameter("conc", Gamma(2.0, 1.0))))
        elif kind == "mixture":
            w = parameter("w", Gamma(2.0, 1.0))
            mu, sd = parameter("mu"), parameter("sd", LogNormal(0, 1))
            mi.sample("y", MixtureSameFamily(Categorical(probs=w), Normal(mu, sd)),
                      sample_shape=[N])
        elif kind == "softmax":
            mi.sample("y", Categorical(logits=d["X"] @ parameter("theta")))
        else:
            eta = parameter("alpha")[d["group"]]
            if kind == "gather_linear":
                eta = eta + d["X"] @ parameter("theta")
            if kind == "gather_slope":
                eta = eta + parameter("beta")[d["group"]] * d["z"]
            mi.sample("y", Normal(eta, parameter("sigma", LogNormal(0, 1))))
    return model


def observed(kind, d, masked):
    """The model's observation (a MaskedTensor when ``masked``), by site name."""
    if kind == "dirichlet":
        return {}
    name, value = ("x", d["rows"]) if kind == "dirichlet_observed" else \
        ("y", d["labels"]) if kind in ("categorical", "softmax") else ("y", d["y"])
    if masked:
        mask = torch.as_tensor(MASK, device=value.device)
        if value.dim() == 2:
            mask = mask[:, None].expand(N, C).contiguous()
        value = torch.masked.as_masked_tensor(value, mask)
    return {name: value}


def row_log_probs(kind, p, d, masked):
    """The site's log density per particle and row, [K, N], in the dtype of ``p``: the model as
    written, over the particle axis."""
    dtype = next(iter(p.values())).dtype
    X, z, y, g = d["X"].to(dtype), d["z"].to(dtype), d["y"].to(dtype), d["group"]
    if kind == "categorical":
        lp = Categorical(logits=p["theta"][:, None, :]).log_prob(d["labels"])
    elif kind == "dirichlet":
        lp = Dirichlet(p["conc"], validate_args=False).log_prob(p["x"])
    elif kind == "dirichlet_observed":
        lp = Dirichlet(p["conc"], validate_args=False).log_prob(d["rows"].to(dtype))
    elif kind == "mixture":
        lp = MixtureSameFamily(Categorical(probs=p["w"][:, None, :]),
                               Normal(p["mu"][:, None, :], p["sd"][:, None, :]),
                               validate_args=False).log_prob(y)
    elif kind == "softmax":
        lp = Categorical(logits=X @ p["theta"]).log_prob(d["labels"])
    else:
        eta = p["alpha"][:, g]
        if kind == "gather_linear":
            eta = eta + p["theta"] @ X.t()
        if kind == "gather_slope":
            eta = eta + p["beta"][:, g] * z
        lp = Normal(eta, p["sigma"][:, None]).log_prob(y)
    if masked:
        lp = torch.where(torch.as_tensor(MASK), lp, torch.zeros((), dtype=dtype))
    return lp


def reference(kind, params, data, masked, frozen):
    """name -> (the gradient of sum_k u_k T_k, the sum over the rows of the absolute terms of
    dT_k), float64, for the parameters that require grad."""
    leaves = {name: t.double().requires_grad_(name != frozen) for name, t in params.items()}
    wanted = [name for name in leaves if name != frozen]
    lp = row_log_probs(kind, leaves, data, masked)
    u = torch.tensor(U, dtype=torch.float64)
    grads = torch.autograd.grad((u[:, None] * lp).sum(), [leaves[n] for n in wanted],
                                retain_graph=True)
    bounds = [torch.zeros_like(g) for g in grads]
    for i in range(N):
        row = torch.autograd.grad(lp[:, i].sum(), [leaves[n] for n in wanted], retain_graph=True)
        for bound, term in zip(bounds, row):
            bound += term.abs()
    return {name: (g, b) for name, g, b in zip(wanted, grads, bounds)}


def close(kind, name, got, want, bound):
    got, err = got.double(), (got.double() - want).abs()
    norm = float(want.abs().max())
    print(f"{kind} d{name}: largest error {float(err.max()):.3g}, max-norm {norm:.3g}")
    if kind == "categorical":       # test_gpu_kernels.py, test_categorical_model_against_oracle
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * norm)
    elif kind.startswith("dirichlet"):   # test_gpu_dirichlet.py, GRAD_RTOL / GRAD_ATOL
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
    elif kind == "mixture":         # test_gpu_mixture.py, test_loss_against_float64
        assert float(err.max()) / norm <= 2e-5, name
    else:   # test_gpu_softmax_linear.py and test_gpu_gather*_site.py: 1e-5 |g0| bound + 1e-7
        u = torch.tensor(U, dtype=torch.float64).abs().reshape((K,) + (1,) * (want.dim() - 1))
        assert bool((err <= 1e-5 * u * bound + 1e-7).all()), (name, err, bound)


@pytest.mark.parametrize("kind,masked,frozen", CASES,
                         ids=[f"{k}{'-masked' if m else ''}{'-no_d' + f if f else ''}"
                              for k, m, f in CASES])
def test_upstream_reaches_every_parameter(device, monkeypatch, kind, masked, frozen):
    params, data = inputs(kind)
    d = {name: t.to(device) for name, t in data.items()}
    samples = {name: t.to(device).requires_grad_(name != frozen) for name, t in params.items()}
    wanted = [name for name in samples if name != frozen]
    scaled = []
    real = _rows._scale_rows
    monkeypatch.setattr(_rows, "_scale_rows", lambda grad, g, g0: scaled.append(tuple(grad.shape))
                        or real(grad, g, g0))

    model = mi.condition(make_model(kind, d), **observed(kind, d, masked))
    trace = particles.trace_particles(model, samples, K, defer_sum=True, defer_slope=True)
    assert trace.fallback == [] and len(trace.sites) == 1
    g0 = float(torch.tensor(-1.0 / K, dtype=torch.float32))
    joint = engine.log_joint(trace, g0, device)
    (site,), shape = trace.sites, KINDS[kind][2]
    if shape is None:
        assert site.launcher is None
    else:   # the fused launch ran, on the entry point of its form
        assert site.launcher is not None
        assert shape == () or (site.launcher.launches, site.launcher.linear,
                               site.launcher.slopes) == (1, *shape)
    (_, holder, _), = joint.pending
    (joint.total * torch.tensor(U, device=device)).sum().backward()
    torch.cuda.synchronize()

    flags = holder["flags"].cpu()
    assert tuple(flags.shape) == (1,) and int(flags[0]) == 0
    joint.raise_on_violation()
    assert len(scaled) == len(wanted), (scaled, wanted)   # none for the parameter without grad
    want = reference(kind, params, data, masked, frozen)
    for name, sample in samples.items():
        if name == frozen:
            assert sample.grad is None
            continue
        assert sample.grad is not None and sample.grad.shape == sample.shape, name
        close(kind, name, sample.grad.cpu(), *want[name])
