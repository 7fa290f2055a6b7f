"""
Time a LowRankMultivariateNormal guide: an eager ELBO evaluation and its backward
of `theta ~ Normal(0, 1)` with D elements, K = 256, R = 16, natively drawn and its entropy native
("native"), natively drawn with torch's own entropy ("torch_entropy": the same code with the
entropy of the family's record in guide.FAMILIES replaced by torch's), and torch's own rsample and
entropy ("torch": the same code with that record's ``accepts`` declining; the table is what
guide.draw and guide.entropy read, so the records are swapped, not the module's functions),
variants alternating in one process, device events; and
mi_lowrank_rsample, mi_lowrank_rsample_backward and mi_lowrank_entropy (value and gradients)
alone. Prints one JSON line per D.
"""
import argparse
import ctypes
import dataclasses
import json
import os
import statistics
import sys

import torch
from torch.distributions import LowRankMultivariateNormal, Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mininf_amd as mi  # noqa: E402
from mininf_amd import _native as nat, guide  # noqa: E402
from mininf_amd.nn import EvidenceLowerBoundLoss, ParameterizedDistribution  # noqa: E402


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def elbo_step(D, R, K, device):
    module = ParameterizedDistribution(
        LowRankMultivariateNormal, loc=torch.zeros(D), cov_factor=0.1 * torch.randn(D, R),
        cov_diag=0.5 * torch.ones(D)).to(device)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=1)

    def model():
        mi.sample("theta", Normal(0, 1), (D,))

    def step():
        module.zero_grad(set_to_none=True)
        loss = loss_fn(model, {"theta": module()})
        loss.backward()
        return loss

    return step, loss_fn


def launches(D, R, K, device):
    loc, d = torch.zeros(D, device=device), 0.5 * torch.ones(D, device=device)
    W = 0.1 * torch.randn(D, R, device=device)
    z, dz = torch.empty(K, D, device=device), torch.randn(K, D, device=device)
    size = ctypes.c_size_t()
    lib = nat.lib()
    nat.check(lib.mi_lowrank_rsample_backward_workspace_bytes(K, D, R, ctypes.byref(size)), "ws")
    ws = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    dloc, dW, dd = torch.empty_like(loc), torch.empty_like(W), torch.empty_like(d)

    def forward():
        nat.check(lib.mi_lowrank_rsample(loc.data_ptr(), W.data_ptr(), d.data_ptr(), K, D, R, 1, 0,
                                         None, 0, 0, None, z.data_ptr(), None), "forward")

    def backward():
        nat.check(lib.mi_lowrank_rsample_backward(
            dz.data_ptr(), D, 1, d.data_ptr(), K, D, R, 1, 0, None, 0, 0, None, ws.data_ptr(),
            size.value, dloc.data_ptr(), dW.data_ptr(), dd.data_ptr(), None), "backward")

    tril = torch.linalg.cholesky(torch.eye(R, device=device) + W.T @ (W / d[:, None]))
    entropy_size = ctypes.c_size_t()
    nat.check(lib.mi_lowrank_entropy_workspace_bytes(D, R, ctypes.byref(entropy_size)), "ws")
    esize = entropy_size.value
    ews = torch.empty(esize, dtype=torch.uint8, device=device)
    H = torch.empty((), device=device)

    def entropy():
        nat.check(lib.mi_lowrank_entropy(
            W.data_ptr(), d.data_ptr(), tril.data_ptr(), D, R, ews.data_ptr(), esize, H.data_ptr(),
            dW.data_ptr(), dd.data_ptr(), None), "entropy")

    return forward, backward, entropy


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", type=int, nargs="+", default=[1024, 16384, 65536])
    parser.add_argument("--rank", type=int, default=16)
    parser.add_argument("--particles", type=int, default=256)
    parser.add_argument("--rounds", type=int, default=12)
    parser.add_argument("--steps", type=int, default=20)
    args = parser.parse_args()
    device = torch.device("cuda")
    families = guide.FAMILIES

    def swapped(**fields):
        """guide.FAMILIES with the LowRankMultivariateNormal record's fields replaced."""
        return tuple(dataclasses.replace(family, **fields) if family.counter == "lowrank"
                     else family for family in families)

    for D in args.sizes:
        R, K = args.rank, args.particles
        native, native_loss = elbo_step(D, R, K, device)
        torch_path, torch_loss = elbo_step(D, R, K, device)
        entropy_path, entropy_loss = elbo_step(D, R, K, device)

        def torch_entropy():   # the native draw with the entropy autograd walks the constructor for
            guide.FAMILIES = swapped(entropy=lambda distribution: distribution.entropy().sum())
            try:
                return entropy_path()
            finally:
                guide.FAMILIES = families

        def declined():
            guide.FAMILIES = swapped(accepts=lambda distribution: False)
            try:
                return torch_path()
            finally:
                guide.FAMILIES = families

        for fn in (native, torch_entropy, declined):
            timed(fn, 10)
        assert native_loss.last_fusions["lowrank_draws"] == 1
        assert native_loss.last_fusions["lowrank_entropies"] == 1
        assert entropy_loss.last_fusions["lowrank_draws"] == 1
        assert entropy_loss.last_fusions["lowrank_entropies"] == 0
        assert torch_loss.last_fusions["lowrank_draws"] == 0
        assert torch_loss.last_fusions["lowrank_entropies"] == 0
        times = {"native": [], "torch_entropy": [], "torch": []}
        for _ in range(args.rounds):
            times["native"].append(timed(native, args.steps))
            times["torch_entropy"].append(timed(torch_entropy, args.steps))
            times["torch"].append(timed(declined, args.steps))
        forward, backward, entropy = launches(D, R, K, device)
        for fn in (forward, backward, entropy):
            timed(fn, 10)
        fwd = [timed(forward, 50) for _ in range(10)]
        bwd = [timed(backward, 50) for _ in range(10)]
        ent = [timed(entropy, 50) for _ in range(10)]
        row = {"D": D, "R": R, "K": K}
        for name, values in (*times.items(), ("forward_launch", fwd), ("backward_launch", bwd),
                             ("entropy_launch", ent)):
            row[name + "_ms"] = {"median": round(statistics.median(values), 4),
                                 "min": round(min(values), 4), "max": round(max(values), 4)}
        # the forward against writing z once: 4 K D bytes
        row["forward_z_gbps"] = round(4 * K * D / (statistics.median(fwd) * 1e-3) / 1e9, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
