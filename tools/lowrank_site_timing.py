"""
Time a factor-analysis likelihood: an eager ELBO evaluation and its backward of

    W ~ Normal(0, 1) [D, R], d ~ LogNormal(0, 1) [D], mu ~ Normal(0, 5) [D],
    x_i ~ LowRankMultivariateNormal(mu, W, d),  i < n

under a mean-field guide at K particles, with the site on mi_lowrank_site_forward / _backward
("native") and with MININF_AMD_LOWRANK_SITE=0 ("torch": the same code with the site on torch's
log_prob inside the particle vmap, the path before the site kernels), the two alternating in one
process, device events; and the site's forward and backward launches alone. Prints one JSON line
per (D, R, n): medians and ranges in milliseconds.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.distributions import LogNormal, LowRankMultivariateNormal, Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mininf_amd as mi  # noqa: E402
from mininf_amd import lowrank_site  # noqa: E402
from mininf_amd.nn import (EvidenceLowerBoundLoss, ParameterizedDistribution,  # noqa: E402
                           ParameterizedFactorizedDistribution)

SWITCH = "MININF_AMD_LOWRANK_SITE"


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def elbo_step(D, R, n, K, device):
    gen = torch.Generator().manual_seed(D * R + n)
    W0 = torch.randn(D, R, generator=gen)
    x = (torch.randn(n, R, generator=gen) @ W0.T + 0.7 * torch.randn(n, D, generator=gen)).to(device)
    module = ParameterizedFactorizedDistribution(
        W=ParameterizedDistribution(Normal, loc=W0.clone(), scale=0.1 * torch.ones(D, R)),
        d=ParameterizedDistribution(LogNormal, loc=-0.7 * torch.ones(D), scale=0.1 * torch.ones(D)),
        mu=ParameterizedDistribution(Normal, loc=torch.zeros(D),
                                     scale=0.1 * torch.ones(D))).to(device)
    loss_fn = EvidenceLowerBoundLoss(num_particles=K, seed=1)
    zero, one, five = (torch.tensor(v, device=device) for v in (0.0, 1.0, 5.0))

    def model():
        W = mi.sample("W", Normal(zero, one), sample_shape=[D, R])
        d = mi.sample("d", LogNormal(zero, one), sample_shape=[D])
        mu = mi.sample("mu", Normal(zero, five), sample_shape=[D])
        mi.sample("x", LowRankMultivariateNormal(mu, W, d), sample_shape=[n])

    conditioned = mi.condition(model, x=x)

    def step():
        module.zero_grad(set_to_none=True)
        loss = loss_fn(conditioned, module())
        loss.backward()
        return loss

    return step


def site_launches(D, R, n, K, device):
    """The site's forward and backward alone in the model's layout: parameters per particle, data
    shared by the particles."""
    W = torch.randn(K, D, R, device=device, requires_grad=True)
    d = (0.3 + torch.rand(K, D, device=device)).requires_grad_()
    mu = torch.randn(K, D, device=device, requires_grad=True)
    x = torch.randn(1, n, D, device=device)
    C = torch.eye(R, device=device) + W.detach().mT @ (W.detach() / d.detach()[..., None])
    L = torch.linalg.cholesky(C)
    g = torch.full((K, n), -1.0 / K, device=device)

    def fn():
        lp, _ = lowrank_site._LowRankSiteLogProb.apply(x, mu, W, d, L)
        torch.autograd.grad(lp, (mu, W, d), g)

    return fn


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", type=int, nargs="+", default=[16, 4, 4096, 256, 64, 4096],
                        help="D R n triples")
    parser.add_argument("--particles", type=int, default=64)
    parser.add_argument("--rounds", type=int, default=6)
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    device = torch.device("cuda")
    K = args.particles
    for D, R, n in zip(args.shapes[0::3], args.shapes[1::3], args.shapes[2::3]):
        native, torch_path = elbo_step(D, R, n, K, device), elbo_step(D, R, n, K, device)

        def declined():
            os.environ[SWITCH] = "0"
            try:
                return torch_path()
            finally:
                del os.environ[SWITCH]

        before = lowrank_site.launches()
        for fn in (native, declined):
            timed(fn, 3)
        assert lowrank_site.launches() == before + 3
        times = {"native": [], "torch": []}
        for _ in range(args.rounds):
            times["native"].append(timed(native, args.steps))
            times["torch"].append(timed(declined, args.steps))
        launch = site_launches(D, R, n, K, device)
        timed(launch, 3)
        alone = [timed(launch, args.steps) for _ in range(args.rounds)]
        row = {"D": D, "R": R, "n": n, "K": K}
        for name, values in (*times.items(), ("site_launches", alone)):
            row[name + "_ms"] = {"median": round(statistics.median(values), 4),
                                 "min": round(min(values), 4), "max": round(max(values), 4)}
        print(json.dumps(row), flush=True)
        del native, torch_path, launch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
