"""
Time the predictive draws: broadcast_samples of the README model (S = 256 samples of
theta, x ~ Bernoulli(theta) over n = 1e6) and of a Poisson(rate[S, n]) site (S = 64, n = 1e6),
natively drawn against torch's own sample (the same code with predictive.supported declining the
family), variants alternating in one process, device events; and each launch alone, back to back.
Prints one JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.distributions import Bernoulli, Beta, Normal, Poisson

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mininf_amd as mi  # noqa: E402
from mininf_amd import _native as nat, predictive  # noqa: E402


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


def case(name, model, states, family, launch, nbytes, args):
    supported = predictive.supported

    def native():
        return mi.broadcast_samples(model, states)

    def declined():
        predictive.supported = lambda d: type(d).__name__ != family and supported(d)
        try:
            return mi.broadcast_samples(model, states)
        finally:
            predictive.supported = supported

    for fn in (native, declined):
        timed(fn, args.warmup)
    predictive.reset_counts()
    native()
    assert predictive.native_draws()[family] == 1
    predictive.reset_counts()
    declined()
    assert predictive.native_draws()[family] == 0
    times = {"native": [], "torch": []}
    for _ in range(args.rounds):
        times["native"].append(timed(native, args.steps))
        times["torch"].append(timed(declined, args.steps))
    timed(launch, args.warmup)
    alone = [timed(launch, 20) for _ in range(args.rounds)]
    row = {"case": name, "native_ms": summary(times["native"]), "torch_ms": summary(times["torch"]),
           "launch_ms": summary(alone),
           "launch_write_gbps": round(nbytes / (statistics.median(alone) * 1e-3) / 1e9, 1)}
    print(json.dumps(row), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--rounds", type=int, default=12)
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=10)
    args = parser.parse_args()
    device = torch.device("cuda")
    lib, n = nat.lib(), args.n

    S = 256
    theta = Beta(2.0, 2.0).sample([S]).to(device)
    out = torch.empty(S * n, dtype=torch.float32, device=device)

    def coin():
        t = mi.sample("theta", Beta(2, 2))
        mi.sample("x", Bernoulli(t), sample_shape=[n])

    def bernoulli_launch():
        nat.check(lib.mi_predictive_sample(nat.PRED_BERNOULLI_PROBS, theta.data_ptr(), 1, 0, None,
                                           0, 0, S, n, 1, 0, out.data_ptr(), None), "sample")

    case("bernoulli S=256", coin, mi.State({"theta": theta}), "Bernoulli", bernoulli_launch,
         4 * S * n, args)

    S = 64
    rate = torch.rand(S, n, device=device) * 20.0 + 0.5   # both regimes in every wave

    def counts():
        log_rate = mi.sample("log_rate", Normal(0, 1), sample_shape=[n])
        mi.sample("y", Poisson(log_rate.exp()))

    def poisson_launch():
        nat.check(lib.mi_predictive_poisson(rate.data_ptr(), n, 1, S, n, 1, 0, out.data_ptr(),
                                            None), "poisson")

    case("poisson S=64", counts, mi.State({"log_rate": rate.log()}), "Poisson", poisson_launch,
         4 * S * n, args)


if __name__ == "__main__":
    main()
