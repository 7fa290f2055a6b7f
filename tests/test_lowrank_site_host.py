"""
The LowRankMultivariateNormal site on the host: the closed form the kernels implement against
torch float64, what ``lowrank_site.enabled`` declines, the three entry points in the header, the
binding and the embedded header, and torch float32's own error on the GPU test's cases (the figures
its bounds are multiples of).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import LowRankMultivariateNormal

from mininf_amd import _native as nat, lowrank_site, switches
from tests import lowrank_site_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi_lowrank_site_workspace_bytes", "mi_lowrank_site_forward",
                "mi_lowrank_site_backward")


@pytest.mark.parametrize("D,R,N,K", [(1, 1, 3, 2), (5, 1, 4, 2), (1, 3, 4, 2), (7, 3, 5, 3),
                                     (33, 31, 2, 1)])
def test_closed_form_is_torch_float64(D, R, N, K):
    case = ref.kernel_case(D, R, N, K)
    args = [case[name] for name in ("value", "loc", "cov_factor", "cov_diag", "g")]
    want = ref.closed_form(*args)
    got = ref.torch_float32(*args, dtype=torch.float64)
    for name in ref.NAMES:
        scale = np.abs(want[name]).max()
        assert np.abs(got[name] - want[name]).max() <= 1e-10 * scale, name
    # the factor the constructor keeps is the one the kernels are handed
    dist = LowRankMultivariateNormal(*(torch.tensor(case[n]).double() for n in ref.PARAMS))
    np.testing.assert_allclose(dist._capacitance_tril.numpy(), want["L"], rtol=1e-12, atol=1e-14)


def test_zero_upstream_rows_are_exact_zeros():
    case = ref.kernel_case(5, 2, 4, 2)
    case["g"][:, 1] = 0.0
    case["value"][:, 1] = np.nan
    want = ref.reference(case)
    for name in ref.GRADS:
        assert np.isfinite(want[name]).all(), name
    assert np.all(want["dvalue"][:, 1] == 0)


class _Sub(LowRankMultivariateNormal):
    pass


def _dist(D=4, R=2, dtype=torch.float32, cls=LowRankMultivariateNormal, rows=None):
    shape = (D, R) if rows is None else (rows, D, R)
    return cls(torch.zeros(D, dtype=dtype), torch.ones(shape, dtype=dtype),
               torch.ones(D, dtype=dtype))


@pytest.mark.parametrize("reason,make", [
    ("type", lambda: _dist(cls=_Sub)),
    ("dtype", lambda: _dist(dtype=torch.float64)),
    ("rank", lambda: _dist(R=nat.LOWRANK_MAX_R + 1)),
    ("size", lambda: _dist(D=nat.LOWRANK_SITE_MAX_D + 1, R=1)),
    ("row batch", lambda: _dist(rows=3)),
    ("host", lambda: _dist()),
])
def test_enabled_declines(reason, make):
    distribution = make()
    assert lowrank_site.why_not(distribution) == reason
    assert not lowrank_site.enabled(distribution)


def test_switch_is_listed_and_on():
    assert switches.SWITCHES["LOWRANK_SITE"][0] is True


def _arguments(text, name):
    match = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
    assert match, name
    return [a.strip() for a in match.group(1).split(",")]


def test_header_binding_and_embedded_header_agree():
    with open(os.path.join(ROOT, "include", "mininf_amd.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "mininf_amd", "csrc", "embedded_header.inc")) as fh:
        embedded = fh.read()
    assert embedded == 'R"MIEMBED(' + header + ')MIEMBED"\n'
    for name in ENTRY_POINTS:
        arguments = _arguments(header, name)
        restype, argtypes = nat._SIGNATURES[name]
        assert len(arguments) == len(argtypes), name
        for text, ctype in zip(arguments, argtypes):
            if "*" in text:
                assert ctype not in (nat.c_i64, ctypes.c_size_t), (name, text)
            elif text.startswith("int64_t"):
                assert ctype is nat.c_i64, (name, text)
            else:
                assert text.startswith("size_t") and ctype is ctypes.c_size_t, (name, text)
    define = re.search(r"#define MI_LOWRANK_SITE_MAX_D \(1 << (\d+)\)", header)
    assert define and 1 << int(define.group(1)) == nat.LOWRANK_SITE_MAX_D
    assert nat.LOWRANK_SITE_MAX_D >= 1024
    assert "#define MI_ABI_VERSION 18" in header and nat.ABI_VERSION == 18


def test_torch_float32_table_is_reproducible():
    worst = {}
    for D, R in ref.KERNEL_DR:
        for _, case in ref.kernel_cases(D, R):
            args = [case[name] for name in ("value", "loc", "cov_factor", "cov_diag", "g")]
            for name, value in ref.fractions(ref.torch_float32(*args), ref.reference(case)).items():
                worst[name] = max(worst.get(name, 0.0), value)
    print(worst)
    assert set(worst) == set(ref.TORCH_F32)
    # (another build of torch may order a float32 sum differently: the same figure to a quarter)
    for name, value in worst.items():
        assert 0.75 * ref.TORCH_F32[name] <= value <= 1.25 * ref.TORCH_F32[name], (name, value)


def test_constructor_cholesky_is_the_only_one_rerouted(monkeypatch):
    """The trace's mode takes the factorisation inside LowRankMultivariateNormal.__init__ (also
    through another mode's frame) and leaves every other torch.linalg.cholesky alone."""
    from torch.overrides import TorchFunctionMode
    taken = []

    def cholesky_ex(A):
        taken.append(tuple(A.shape))
        return torch.linalg.cholesky_ex(A)

    monkeypatch.setattr(lowrank_site.ConstructorCholesky, "_native", staticmethod(lambda A: True))
    monkeypatch.setattr(lowrank_site.mvn, "cholesky_ex", cholesky_ex)

    class Passing(TorchFunctionMode):
        def __torch_function__(self, func, types, args=(), kwargs=None):
            return func(*args, **(kwargs or {}))

    with lowrank_site.ConstructorCholesky():
        torch.linalg.cholesky(torch.eye(3))
        assert taken == []
        plain = _dist(D=4, R=2)
        assert taken == [(2, 2)]
        with Passing():
            _dist(D=4, R=3)
        assert taken == [(2, 2), (3, 3)]
        torch.distributions.MultivariateNormal(torch.zeros(3), covariance_matrix=torch.eye(3))
        assert taken == [(2, 2), (3, 3)]
    want = LowRankMultivariateNormal(torch.zeros(4), torch.ones(4, 2), torch.ones(4))
    assert torch.equal(plain._capacitance_tril, want._capacitance_tril)
    # off the device, over the rank or with the switch off nothing is taken
    monkeypatch.undo()
    assert not lowrank_site.ConstructorCholesky._native(torch.eye(3))
