"""
Time a marginalised Normal-mixture likelihood: an eager ELBO evaluation and its
backward of

    w ~ Dirichlet(1_C), mu_c ~ Normal(0, 5), sd_c ~ LogNormal(0, 1),
    x_i ~ MixtureSameFamily(Categorical(w), Normal(mu, sd)),  i < n

under a mean-field guide at K = 256, with the mixture site on mi_mixture_normal_forward ("native")
and with the classification declining ("torch": the same code with the site on torch's log_prob
inside the particle vmap, the path before the site kernel), the two alternating in one process,
device events; and the site launch alone with its bytes over its time. Prints one JSON line per
(C, n).
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.distributions import Categorical, Dirichlet, LogNormal, MixtureSameFamily, Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mininf_amd as mi  # noqa: E402
from mininf_amd import engine, particles  # noqa: E402
from mininf_amd.nn import (EvidenceLowerBoundLoss, ParameterizedDistribution,  # noqa: E402
                           ParameterizedFactorizedDistribution)
from mininf_amd.particles import SiteRecord  # noqa: E402

STREAM_TBPS = 6.3   # the streaming figure the launch's bytes over its time are set against


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def elbo_step(C, n, K, device):
    gen = torch.Generator().manual_seed(C * n)
    centres = torch.linspace(-6.0, 6.0, C)
    x = (centres[torch.randint(0, C, (n,), generator=gen)] +
         0.5 * torch.randn(n, generator=gen)).to(device)
    module = ParameterizedFactorizedDistribution(
        w=ParameterizedDistribution(Dirichlet, concentration=2.0 * torch.ones(C)),
        mu=ParameterizedDistribution(Normal, loc=centres.clone(), scale=0.3 * torch.ones(C)),
        sd=ParameterizedDistribution(LogNormal, loc=-0.5 * torch.ones(C),
                                     scale=0.2 * torch.ones(C))).to(device)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=1)
    ones = torch.ones(C, device=device)
    zero, one, five = (torch.tensor(v, device=device) for v in (0.0, 1.0, 5.0))

    def model():
        w = mi.sample("w", Dirichlet(ones))
        mu = mi.sample("mu", Normal(zero, five), sample_shape=[C])
        sd = mi.sample("sd", LogNormal(zero, one), sample_shape=[C])
        mi.sample("x", MixtureSameFamily(Categorical(probs=w), Normal(mu, sd)), sample_shape=[n])

    conditioned = mi.condition(model, x=x)

    def step():
        module.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, module())
        loss.backward()
        return loss

    return step


def site_launch(C, n, K, device):
    """The launch alone in the model's layout: parameters [K, C] shared by the rows, data shared by
    the particles; returns (fn, bytes moved)."""
    logits = torch.randn(K, 1, C, device=device).expand(K, n, C)
    loc = (3 * torch.randn(K, 1, C, device=device)).expand(K, n, C)
    scale = (0.3 + torch.rand(K, 1, C, device=device)).expand(K, n, C)
    for t in (logits, loc, scale):
        t.requires_grad_()
    value = torch.randn(1, n, device=device).expand(K, n)
    site = SiteRecord("x", "mixture_normal", [], torch.Size([n]), 1.0, None, "MixtureSameFamily")

    def fn():
        engine._run_mixture_normal(site, -1.0 / K, (logits, loc, scale), value, None,
                                   (True, True, True, False))

    # read: the data once per particle (from the caches after the first) and the [K, C] parameters;
    # written: three [K, n, C] gradients and the rows' fp64 densities
    moved = 4 * n + 3 * 4 * K * C + 3 * 4 * K * n * C + 8 * K * n
    return fn, moved


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--components", type=int, nargs="+", default=[4, 64])
    parser.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    parser.add_argument("--particles", type=int, default=256)
    parser.add_argument("--rounds", type=int, default=12)
    parser.add_argument("--steps", type=int, default=20)
    args = parser.parse_args()
    device = torch.device("cuda")
    kernel_mixture = particles._kernel_mixture
    K = args.particles
    for C in args.components:
        for n in args.sizes:
            native, torch_path = elbo_step(C, n, K, device), elbo_step(C, n, K, device)

            def declined():
                particles._kernel_mixture = lambda distribution: False
                try:
                    return torch_path()
                finally:
                    particles._kernel_mixture = kernel_mixture

            for fn in (native, declined):
                timed(fn, 10)
            times = {"native": [], "torch": []}
            for _ in range(args.rounds):
                times["native"].append(timed(native, args.steps))
                times["torch"].append(timed(declined, args.steps))
            launch, moved = site_launch(C, n, K, device)
            timed(launch, 10)
            alone = [timed(launch, 20) for _ in range(10)]
            row = {"C": C, "n": n, "K": K}
            for name, values in (*times.items(), ("site_launch", alone)):
                row[name + "_ms"] = {"median": round(statistics.median(values), 4),
                                     "min": round(min(values), 4), "max": round(max(values), 4)}
            tbps = moved / (statistics.median(alone) * 1e-3) / 1e12
            row["site_launch_tbps"] = round(tbps, 3)
            row["site_launch_of_stream"] = round(tbps / STREAM_TBPS, 3)
            print(json.dumps(row), flush=True)
            del native, torch_path, launch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
