"""
Time the one-noise-word guide factors: an eager ELBO evaluation and its backward of
`sigma ~ Gamma(2, 2)` (D elements), `y ~ Normal(0, sigma)` under a D-element LogNormal guide at
K = 256, natively drawn against torch's own rsample and entropy (the same code with the
``accepts`` of the family's record in guide.FAMILIES declining; the table is what guide.draw and
guide.entropy read, so the record is swapped, not guide.native_elementwise), variants alternating
in one process, device events; and
mi_elementwise_rsample + mi_elementwise_rsample_backward alone for every family at K = 4096,
N = 65536 (1 GiB of draws), as achieved bytes per second: z written, dz read. Prints one JSON line
per measurement.
"""
import argparse
import ctypes
import dataclasses
import json
import os
import statistics
import sys

import torch
from torch.distributions import Gamma, LogNormal, Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mininf_amd as mi  # noqa: E402
from mininf_amd import _native as nat, guide  # noqa: E402
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution  # noqa: E402

FAMILIES = {"exponential": nat.PRED_EXPONENTIAL, "laplace": nat.PRED_LAPLACE,
            "cauchy": nat.PRED_CAUCHY, "half_cauchy": nat.PRED_HALF_CAUCHY,
            "half_normal": nat.PRED_HALF_NORMAL, "log_normal": nat.PRED_LOG_NORMAL}
TWO = ("laplace", "cauchy", "log_normal")


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4),
            "max": round(max(values), 4)}


def elbo_step(D, K, device):
    module = ParameterizedDistribution(LogNormal, loc=torch.zeros(D),
                                       scale=0.3 * torch.ones(D)).to(device)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=1)
    y = torch.randn(D, generator=torch.Generator().manual_seed(0)).to(device)

    def model():
        sigma = mi.sample("sigma", Gamma(2.0, 2.0), (D,))
        mi.sample("y", Normal(0.0, sigma))

    conditioned = mi.condition(model, y=y)

    def step():
        module.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, {"sigma": module()})
        loss.backward()
        return loss

    return step, loss_fn


def launches(family, K, N, device):
    a = 0.5 + torch.rand(N, device=device)
    b = 0.05 + 0.2 * torch.rand(N, device=device) if family in TWO else None
    z, dz = torch.empty(K, N, device=device), torch.randn(K, N, device=device)
    size = ctypes.c_size_t()
    lib, code = nat.lib(), FAMILIES[family]
    nat.check(lib.mi_elementwise_rsample_backward_workspace_bytes(K, N, ctypes.byref(size)), "ws")
    ws = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    da = torch.empty(N, device=device)
    db = torch.empty(N, device=device) if b is not None else None

    def forward():
        nat.check(lib.mi_elementwise_rsample(code, a.data_ptr(), 1, nat.ptr(b), 1, K, N, 1, 0,
                                             None, 0, 0, None, z.data_ptr(), None), "forward")

    def backward():
        nat.check(lib.mi_elementwise_rsample_backward(
            code, dz.data_ptr(), N, 1, a.data_ptr(), 1, nat.ptr(b), 1, K, N, 1, 0, None, 0, 0,
            None, ws.data_ptr(), size.value, da.data_ptr(), nat.ptr(db), None), "backward")

    return forward, backward


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    parser.add_argument("--particles", type=int, default=256)
    parser.add_argument("--rounds", type=int, default=12)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--launch-particles", type=int, default=4096)
    parser.add_argument("--launch-elements", type=int, default=65536)
    args = parser.parse_args()
    device = torch.device("cuda")
    families = guide.FAMILIES
    declining = tuple(dataclasses.replace(family, accepts=lambda distribution: False)
                      if family.counter == "elementwise" else family for family in families)
    for D in args.sizes:
        K = args.particles
        native, native_loss = elbo_step(D, K, device)
        torch_path, torch_loss = elbo_step(D, K, device)

        def declined():
            guide.FAMILIES = declining
            try:
                return torch_path()
            finally:
                guide.FAMILIES = families

        for fn in (native, declined):
            timed(fn, 10)
        assert native_loss.last_fusions["elementwise_draws"] == 1
        assert torch_loss.last_fusions["elementwise_draws"] == 0
        times = {"native": [], "torch": []}
        for _ in range(args.rounds):
            times["native"].append(timed(native, args.steps))
            times["torch"].append(timed(declined, args.steps))
        row = {"eager_step": True, "D": D, "K": K}
        row.update({name + "_ms": summary(values) for name, values in times.items()})
        print(json.dumps(row), flush=True)
    K, N = args.launch_particles, args.launch_elements
    for family in FAMILIES:
        forward, backward = launches(family, K, N, device)
        for fn in (forward, backward):
            timed(fn, 5)
        fwd = [timed(forward, 10) for _ in range(args.rounds)]
        bwd = [timed(backward, 10) for _ in range(args.rounds)]
        row = {"launches": family, "K": K, "N": N, "forward_ms": summary(fwd),
               "backward_ms": summary(bwd),
               # z written once, dz read once: 4 K N bytes each
               "forward_z_gbps": round(4 * K * N / (statistics.median(fwd) * 1e-3) / 1e9, 1),
               "backward_dz_gbps": round(4 * K * N / (statistics.median(bwd) * 1e-3) / 1e9, 1)}
        print(json.dumps(row), flush=True)
        del forward, backward
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
