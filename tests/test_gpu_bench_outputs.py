"""
bench.py's plain run and ``--dump-outputs`` on the GPU: the line of a plain run carries the step
time and none of the ``--full`` measurements, the dump holds the last timed step's loss, guide
parameters and gradients as float32 arrays, and two runs with the same arguments write the same
arrays (the inputs and the number of steps before the timed ones depend on the arguments alone).

The two runs (C1: n = 10, one particle) are child processes started together once per session.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

NAMES = ["loss"] + [f"{kind}.distribution_parameters.concentration{i}"
                    for kind in ("param", "grad") for i in (0, 1)]


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dirs = [str(tmp_path_factory.mktemp(f"dump{i}") / "out") for i in range(2)]
    children = [subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "bench.py"),
                                  "--gpus", "1", "--config", "c1", "--steps", "4", "--warmup", "2",
                                  "--dump-outputs", d], env=env, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for d in dirs]
    results = []
    for child, d in zip(children, dirs):
        stdout, stderr = child.communicate(timeout=240)
        assert child.returncode == 0, (stdout[-3000:], stderr[-3000:])
        results.append((json.loads(stdout.strip().splitlines()[-1]), d))
    return results


def test_plain_line_has_the_step_time_and_no_full_measurements(runs):
    line, _ = runs[0]
    assert line["steps"] == 4 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["unit"] == "site-log_prob evals/s"
    assert "hipGraph replay (4 steps per replay)" == line["config"]["step_mode"]
    for key in ("roofline", "cpu_baseline", "other_configs"):
        assert key not in line
    for key in ("eager_ms_per_step", "reducible_floor_ms_per_step"):
        assert key not in line["config"]


def test_dump_holds_the_last_steps_outputs(runs):
    line, directory = runs[0]
    assert sorted(os.listdir(directory)) == sorted(name + ".npy" for name in NAMES)
    arrays = {name: np.load(os.path.join(directory, name + ".npy")) for name in NAMES}
    for name, array in arrays.items():
        assert array.dtype == np.float32 and array.shape == () and np.isfinite(array), name
    assert float(arrays["loss"]) == line["config"]["final_loss"]


def test_same_arguments_give_the_same_outputs(runs):
    (_, first), (_, second) = runs
    for name in NAMES:
        a = np.load(os.path.join(first, name + ".npy"))
        b = np.load(os.path.join(second, name + ".npy"))
        assert np.array_equal(a, b), (name, a, b)
