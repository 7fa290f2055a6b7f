"""
The layout of the ``mininf_amd.engine`` package (host only -- no GPU): the engine's layers live in
private submodules, and everything that reaches into the engine from outside keeps working:

* every attribute the package, the tests, ``bench.py`` and ``tools/`` read resolves on
  ``mininf_amd.engine``;
* any submodule can be the first thing of the package a process imports;
* there is one held step (``_held._PENDING``), whichever module asks for it;
* ``attach_optimizer`` writes into the dict ``mininf_amd.engine.LAST_FUSIONS`` is bound to when it
  runs (``elbo()`` rebinds it on every call, and the loss keeps that dict).
"""
import os
import subprocess
import sys

import pytest
import torch

from mininf_amd import _native as nat
from mininf_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every `engine.<name>` read in mininf_amd/, tests/, bench.py and tools/
USED_NAMES = (
    "FAMILY_CODES", "KERNEL_TIMER", "LAST_FUSIONS", "LogJoint", "PendingGrad", "_ElboPlan",
    "_FUSED_ADAM_MAX_NUMEL", "_GroupLauncher", "_PendingStep", "_View", "_defer_step",
    "_lazy_uses", "_run_dirichlet", "_to_device", "attach_optimizer", "claim_linear_draws",
    "discard_pending_step", "elbo", "entropy_factors", "flush_pending_step", "fold_linear_priors",
    "fold_priors", "grad_meta", "log_joint", "pending_step", "plan_absorption", "plan_groups",
    "plan_linear", "release_unsafe_claims", "torch_function_flush")

SUBMODULES = ("_operands", "_groups", "_rows", "_linear", "_plan", "_absorb", "_elbo_plan", "_held")


@pytest.mark.parametrize("name", USED_NAMES)
def test_used_names_resolve_on_the_package(name):
    getattr(engine, name)


def test_submodule_list_is_the_directory():
    found = {f[:-3] for f in os.listdir(os.path.dirname(engine.__file__))
             if f.startswith("_") and f.endswith(".py") and f != "__init__.py"}
    assert found == set(SUBMODULES)


@pytest.mark.parametrize("name", SUBMODULES)
def test_submodule_imports_first(name):
    code = (f"import mininf_amd.engine.{name} as m, sys\n"
            "e = sys.modules['mininf_amd.engine']\n"
            f"assert e.{name} is m and e.KERNEL_TIMER is None and e.LAST_FUSIONS == {{}}\n"
            "assert callable(e.elbo) and callable(e.log_joint)\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


class _Launch:
    def __init__(self):
        self.calls = []

    def __call__(self, adam):
        self.calls.append(adam)
        return 0


@pytest.fixture
def held():
    """A stand-in launch held for the optimizer, writing the gradient ``g``."""
    engine.discard_pending_step()
    g = torch.zeros(8)
    launch = _Launch()
    assert engine._defer_step(launch, "stand-in", [[g]], (g,))
    yield launch, g
    engine.discard_pending_step()


def test_one_pending_step(held):
    step = engine.pending_step()
    assert step is not None
    assert engine._held.pending_step() is step and engine._held._PENDING is step
    engine.flush_pending_step()
    assert engine.pending_step() is None and engine._held._PENDING is None
    assert held[0].calls == [None]


def test_attach_optimizer_writes_the_current_fusion_dict(held, monkeypatch):
    launch, g = held
    fusions = {}
    monkeypatch.setattr(engine, "LAST_FUSIONS", fusions)
    desc = nat.Adam()
    desc.num = 1
    desc.tensors[0].numel = 8
    desc.tensors[0].grad = g.data_ptr()
    assert engine.attach_optimizer(desc, [g])
    assert launch.calls == [desc]
    assert engine.LAST_FUSIONS is fusions and fusions == {"optimizer_step": 1}
