"""
The site families beyond the first eight (Exponential, Laplace, Cauchy, HalfNormal, HalfCauchy,
LogNormal and its spelled-out TransformedDistribution, StudentT, Binomial, NegativeBinomial), host
side: how ``particles.classify`` maps them, what stays on the torch path, that the Python constants
and the embedded header agree with ``enum mi_family`` of include/mininf_amd.h, that ``mi_site``
kept its layout, and that the site programs specialised for them compile (hiprtc needs no device).
No kernel is launched here.
"""
import ctypes
import os
import re

import pytest
import torch
from torch.distributions import AffineTransform, Binomial, Cauchy, Exponential, ExpTransform, \
    Gamma, HalfCauchy, HalfNormal, Laplace, LogNormal, NegativeBinomial, Normal, StudentT, \
    TransformedDistribution

import mininf_amd as mi
from mininf_amd import _native as nat, engine, particles
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mininf_amd.h")
EMBEDDED = os.path.join(ROOT, "mininf_amd", "csrc", "embedded_header.inc")

NEW_CODES = {"exponential": 7, "laplace": 8, "cauchy": 9, "half_normal": 10, "half_cauchy": 11,
             "log_normal": 12, "student_t": 13, "binomial": 14, "negative_binomial": 15}


def header_enum(path):
    """name -> value of ``enum mi_family`` as written in `path`."""
    body = re.search(r"enum mi_family \{(.*?)\};", open(path).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {name: int(value) for name, value in re.findall(r"(MI_\w+)\s*=\s*(\d+)", body)}


def same(got, want):
    return isinstance(got, torch.Tensor) and got.shape == want.shape and bool((got == want).all())


def test_classify_maps_the_ten_distributions():
    a, b = torch.tensor([0.5, 1.5, -2.0]), torch.tensor([1.0, 2.0, 0.25])
    n, logits = torch.tensor([3, 7, 0]), torch.tensor([-1.0, 0.5, 8.0])
    cases = [
        (Exponential(b), "exponential", [b]),
        (Laplace(a, b), "laplace", [a, b]),
        (Cauchy(a, b), "cauchy", [a, b]),
        (HalfNormal(b), "half_normal", [b]),
        (HalfCauchy(b), "half_cauchy", [b]),
        (LogNormal(a, b), "log_normal", [a, b]),
        (TransformedDistribution(Normal(a, b), ExpTransform()), "log_normal", [a, b]),
        (TransformedDistribution(Normal(a, b), [ExpTransform()]), "log_normal", [a, b]),
        (StudentT(4.0, a, b), "student_t", [a, b]),
        (StudentT(torch.tensor([2.5]), a, b), "student_t", [a, b]),
        (Binomial(n, logits=logits), "binomial", [n.float(), logits]),
        (NegativeBinomial(b, logits=logits), "negative_binomial", [b, logits]),
    ]
    for distribution, family, roles in cases:
        got_family, got_roles = particles.classify(distribution)
        assert got_family == family, distribution
        assert len(got_roles) == len(roles), family
        for got, want in zip(got_roles, roles):
            assert same(got, want), (family, got, want)


def test_count_families_pass_torchs_own_logits():
    """A `probs` construction is read through torch's lazy probs_to_logits (its clamp, its
    autograd), as Binomial.log_prob and NegativeBinomial.log_prob read it."""
    probs = torch.tensor([0.0, 0.25, 1.0], requires_grad=True)
    for distribution in (Binomial(torch.tensor([4, 4, 4]), probs=probs),
                         NegativeBinomial(torch.tensor([2.5, 2.5, 2.5]), probs=probs * 0.5)):
        family, roles = particles.classify(distribution)
        assert family in ("binomial", "negative_binomial")
        assert roles[1] is distribution.logits and roles[1].requires_grad
        assert torch.isfinite(roles[1]).all()   # probs 0 and 1 are clamped by torch


def test_student_t_df_is_recorded_and_other_dfs_stay_on_torch():
    a, b = torch.zeros(3), torch.ones(3)
    assert particles._classify(StudentT(4.0, a, b))[2] == 4.0
    assert particles._classify(StudentT(torch.tensor(2.5), a, b))[2] == 2.5
    assert particles.classify(StudentT(torch.tensor(4.0, requires_grad=True), a, b)) == \
        ("torch", [])
    assert particles.classify(StudentT(torch.tensor([3.0, 4.0, 5.0]), a, b)) == ("torch", [])
    assert particles.classify(StudentT(torch.tensor([4.0, 4.0, 4.0]), a, b)) == ("torch", [])
    # three host numbers (a constant prior): a torch site, whose host constants a captured step
    # pins as device copies (tests/test_gpu_graph.py); one tensor parameter makes it native
    assert particles.classify(StudentT(3.0, 0.0, 1.0)) == ("torch", [])
    assert particles.classify(StudentT(3.0, torch.zeros(()), torch.ones(()))) == ("torch", [])
    assert particles.classify(StudentT(3.0, 0.0, b))[0] == "student_t"


def test_what_stays_on_the_torch_path():
    a, b = torch.zeros(3), torch.ones(3)

    class MyLaplace(Laplace):
        def log_prob(self, value):
            return super().log_prob(value) * 2

    class MyLogNormal(LogNormal):
        def log_prob(self, value):
            return super().log_prob(value) - 1

    assert particles.classify(MyLaplace(a, b)) == ("torch", [])
    assert particles.classify(MyLogNormal(a, b)) == ("torch", [])
    assert particles.classify(TransformedDistribution(
        Normal(a, b), [ExpTransform(), AffineTransform(1.0, 2.0)])) == ("torch", [])
    assert particles.classify(TransformedDistribution(Laplace(a, b), ExpTransform())) == \
        ("torch", [])


def test_torch_path_site_still_traces():
    """Everything outside the StudentT rule still works: the site is evaluated by torch inside
    the trace, with torch's density."""
    K, n = 4, 5
    y = torch.randn(n)
    df = torch.tensor([3.0, 4.0, 5.0, 6.0, 7.0])

    def model():
        z = mi.sample("z", Normal(0, 1), sample_shape=[n])
        mi.sample("y", StudentT(df, z, 1.0))
    z = torch.randn(K, n)
    trace = particles.trace_particles(mi.condition(model, y=y), {"z": z}, K)
    assert [site.name for site in trace.sites] == ["z"]
    assert [name for name, _ in trace.fallback] == ["y"]
    want = StudentT(df, z, 1.0).log_prob(y).sum(-1)
    torch.testing.assert_close(trace.fallback[0][1], want)


def test_constants_agree_with_the_header_enum():
    enum = header_enum(HEADER)
    assert {name: enum["MI_" + name.upper()] for name in NEW_CODES} == NEW_CODES
    for name, code in engine.FAMILY_CODES.items():
        assert enum["MI_" + name.upper()] == code == getattr(nat, name.upper()), name
    assert sorted(engine.FAMILY_CODES.values()) == sorted(enum.values())


def test_embedded_header_holds_the_same_enum():
    nat.lib()   # (the build regenerates csrc/embedded_*.inc)
    assert header_enum(EMBEDDED) == header_enum(HEADER)
    text = open(EMBEDDED).read()
    assert text.startswith('R"MIEMBED(') and text[len('R"MIEMBED('):-len(')MIEMBED"\n')] == \
        open(HEADER).read()


def test_site_struct_keeps_its_layout():
    sizes = [ctypes.c_size_t() for _ in range(3)]
    assert nat.lib().mi_struct_sizes(*[ctypes.byref(s) for s in sizes]) == 0
    assert sizes[1].value == ctypes.sizeof(nat.Site) == 64
    # `extra` sits where the padding word was: after constant[3], before the mask pointer
    assert nat.Site.extra.offset == nat.Site.constant.offset + 12 == 28
    assert nat.Site.extra.size == 4 and nat.Site.mask.offset == 32
    assert nat.Site().extra == 0.0   # a zero-initialised descriptor stays valid
    assert nat.lib().mi_abi_version(ctypes.create_string_buffer(16), 16) == 18


def scale_priors(n):
    def model():
        sigma = mi.sample("sigma", HalfCauchy(1.0))
        tau = mi.sample("tau", HalfNormal(2.0))
        lam = mi.sample("lam", Exponential(0.5))
        s = mi.sample("s", LogNormal(0.0, 1.0))
        mi.sample("y", Cauchy(lam, sigma + tau + s), sample_shape=[n])
    return model


def robust(n):
    def model():
        sigma = mi.sample("sigma", Gamma(2.0, 2.0))
        z = mi.sample("z", Laplace(0.0, 1.0), sample_shape=[n])
        mi.sample("y", StudentT(4.0, z, sigma))
    return model


def counts(n, x, total):
    def model():
        a = mi.sample("a", Normal(0, 1))
        b = mi.sample("b", Normal(0, 1))
        r = mi.sample("r", Gamma(2.0, 1.0))
        with mi.batch(1000):
            mi.sample("c", NegativeBinomial(r, logits=a + b * x))
        mi.sample("m", Binomial(total, probs=torch.sigmoid(a + b * x)))
    return model


@pytest.mark.parametrize("case", ["scale_priors", "robust", "counts"])
def test_site_programs_of_the_new_families_compile(case):
    K, n = 8, 37
    positive = lambda *shape: torch.rand(K, *shape).add(0.5).requires_grad_()   # noqa: E731
    if case == "scale_priors":
        model = mi.condition(scale_priors(n), y=torch.randn(n))
        samples = {name: positive() for name in ("sigma", "tau", "lam", "s")}
    elif case == "robust":
        mask = torch.rand(n) > 0.3
        model = mi.condition(robust(n), y=torch.masked.as_masked_tensor(torch.randn(n), mask))
        samples = {"sigma": positive(), "z": torch.randn(K, n, requires_grad=True)}
    else:
        x, total = torch.randn(n), torch.randint(0, 9, (n,))
        model = mi.condition(counts(n, x, total), c=torch.randint(0, 6, (n,)).float(),
                             m=(total // 2).float())
        samples = {"a": torch.randn(K, requires_grad=True),
                   "b": torch.randn(K, requires_grad=True), "r": positive()}
    trace = particles.trace_particles(model, samples, K)
    assert trace.fallback == []
    launchers, _ = engine.plan_groups(trace, -1.0 / K, torch.device("cpu"))
    assert launchers
    names = set()
    for launcher in launchers:
        for grads in (True, False):
            launcher.compile_check(grads)
        group, _ = launcher.describe(True, query=True)
        for index, (site, _, _) in enumerate(launcher.sites):
            names.add(site.family)
            assert group.sites[index].family == engine.FAMILY_CODES[site.family]
            assert group.sites[index].extra == (4.0 if site.family == "student_t" else 0.0)
    expected = {"scale_priors": {"half_cauchy", "half_normal", "exponential", "log_normal",
                                 "cauchy"},
                "robust": {"gamma", "laplace", "student_t"},
                "counts": {"normal", "gamma", "negative_binomial", "binomial"}}[case]
    assert names == expected
