"""
The run-time switches (``mininf_amd.switches``, host only -- no GPU): one reader with the meaning
the scattered ``os.environ.get`` calls had, read at call time, used by every module of the package,
and one table that names every ``MININF_AMD_*`` variable the sources mention.
"""
import os
import re

import pytest

import mininf_amd
from mininf_amd import switches

PACKAGE = os.path.dirname(os.path.abspath(mininf_amd.__file__))
NAME = "MININF_AMD_LAYOUT_TEST_SWITCH"


def _sources(suffixes):
    for folder, _, files in os.walk(PACKAGE):
        for f in files:
            if f.endswith(suffixes):
                path = os.path.join(folder, f)
                with open(path, encoding="utf-8") as handle:
                    yield os.path.relpath(path, PACKAGE), handle.read()


@pytest.mark.parametrize("value", [None, "", "0", "1", "2"])
def test_semantics_are_the_old_expressions(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(NAME, raising=False)
    else:
        monkeypatch.setenv(NAME, value)
    name = NAME[len("MININF_AMD_"):]
    # default on: the old `!= "0"` to enable and `== "0"` to disable
    assert switches.enabled(name) == (os.environ.get(NAME, "1") != "0")
    assert switches.enabled(name, default=True) == (not os.environ.get(NAME, "1") == "0")
    # default off: the old `!= "1"` to leave disabled
    assert switches.enabled(name, default=False) == (not os.environ.get(NAME, "0") != "1")
    assert switches.enabled(name) == (value != "0")
    assert switches.enabled(name, default=False) == (value == "1")


def test_read_at_call_time(monkeypatch):
    name = NAME[len("MININF_AMD_"):]
    monkeypatch.delenv(NAME, raising=False)
    assert switches.enabled(name) and not switches.enabled(name, default=False)
    monkeypatch.setenv(NAME, "0")
    assert not switches.enabled(name)
    monkeypatch.setenv(NAME, "1")
    assert switches.enabled(name) and switches.enabled(name, default=False)


def test_no_stray_reads():
    stray = []
    for path, text in _sources((".py",)):
        if path == "switches.py":
            continue
        for number, line in enumerate(text.splitlines(), 1):
            if 'environ.get("MININF_AMD_' in line or "environ.get('MININF_AMD_" in line:
                stray.append((path, number, line.strip()))
    assert len(stray) == 1 and stray[0][0] == "_native.py" and "MININF_AMD_LIB" in stray[0][2], stray


def test_table_is_complete():
    listed = set(switches.SWITCHES) | set(switches.ELSEWHERE)
    assert not set(switches.SWITCHES) & set(switches.ELSEWHERE)
    missing = set()
    for path, text in _sources((".py", ".cpp", ".hip", ".hpp")):
        for name in re.findall(r"MININF_AMD_([A-Z_]+)", text):
            if name not in listed:
                missing.add((path, name))
    assert not missing, sorted(missing)


def test_call_sites_use_the_table_defaults():
    """Every ``switches.enabled("X"[, default=False])`` in the package names a listed switch with
    the default the table gives it."""
    calls = []
    for path, text in _sources((".py",)):
        calls += [(path, name, tail) for name, tail in
                  re.findall(r'switches\.enabled\("([A-Z_]+)"([^)]*)\)', text)]
    for path, name, tail in calls:
        assert name in switches.SWITCHES, (path, name)
        assert switches.SWITCHES[name][0] == ("default=False" not in tail), (path, name)
    assert {name for _, name, _ in calls} == set(switches.SWITCHES)
