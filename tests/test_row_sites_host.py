"""
The row sites' plumbing on the host (no GPU): ``engine._rows._RowSiteFn`` around a stand-in
launcher -- how it splits its inputs, what it keeps and what its backward returns and rescales --
and ``graph._release_graph_refs``, which drops a site's launcher with its other references.
"""
import types

import torch

from mininf_amd import graph
from mininf_amd.engine import _rows
from mininf_amd.particles import SiteRecord


class _Launcher:
    """Speculative gradients g0 * 2 for the parameters that require grad; total = sum of them."""
    def __init__(self):
        self.calls = []

    def run(self, params, g0, flags=None):
        self.calls.append((params, g0, flags))
        total = sum(2.0 * p.detach().reshape(p.shape[0], -1).sum(1) for p in params)
        grads = tuple(torch.full_like(p, 2.0 * g0) if p.requires_grad else None for p in params)
        return total, grads, None, torch.zeros(1, dtype=torch.int32)


def _site(launcher=None):
    site = SiteRecord("y", "normal", [], torch.Size([4]), 1.0, None, "Normal")
    site.launcher = launcher
    return site


def test_autograd_function_around_a_launcher(monkeypatch):
    scaled = []

    def scale_rows(grad, g, g0):   # mi_scale_rows on the host
        scaled.append(grad)
        grad *= (g / g0).reshape((-1,) + (1,) * (grad.dim() - 1))
    monkeypatch.setattr(_rows, "_scale_rows", scale_rows)
    a = torch.randn(3, 2, requires_grad=True)
    b = torch.randn(3)
    c = torch.randn(3, 2, 2, requires_grad=True)
    value, holder, launcher = torch.randn(4), {}, _Launcher()
    total = _rows._RowSiteFn.apply(_site(launcher), holder, -0.25, a, b, c, value, None)
    (params, g0, flags), = launcher.calls
    assert [p.shape for p in params] == [a.shape, b.shape, c.shape] and g0 == -0.25
    assert flags is None and holder["flags"].tolist() == [0]
    u = torch.tensor([0.5, -2.0, 3.0])
    (total * u).sum().backward()
    assert len(scaled) == 2 and b.grad is None   # nothing rescaled for the one without grad
    assert torch.equal(a.grad, (2.0 * u)[:, None].expand(3, 2))
    assert torch.equal(c.grad, (2.0 * u)[:, None, None].expand(3, 2, 2))


def test_release_graph_refs_drops_the_launcher():
    site = _site(_Launcher())
    site.tensors = [torch.zeros(3, 4)]
    joint = types.SimpleNamespace(total=torch.zeros(3), pending=[("normal", {}, [site])])
    graph._release_graph_refs([joint])
    assert site.launcher is None and site.tensors == [] and joint.total is None
