"""
ms_per_step of a regression on X @ theta with a count (or Bernoulli / Normal) likelihood at the C3
and C4 shapes, measured by bench.py's own run_config (graph replay, warm-up, timed replays, and with
--full the span-stamped site kernel): bench.workload is replaced for the run, bench.py is not edited.

  python tools/count_regression_bench.py --shape c3 --likelihood poisson
  python tools/count_regression_bench.py --shape c4 --likelihood bernoulli --full

Shapes: c3 = N 1e6, P 32, K 256, whole data per step; c4 = 1e7 rows resident, DeviceDataLoader
minibatches of 65536 (shuffled), K 256. Prints bench.py's JSON line (ms_per_step, fusions; with
--full the roofline's kernel_ms). --root DIR imports bench.py and the package from another checkout
(e.g. the parent commit, which materialises the predictor of a count likelihood), so that both builds
can be run alternately in one session.
"""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("c3", "c4"), default="c3")
    ap.add_argument("--likelihood", default="poisson",
                    choices=("poisson", "binomial", "negative_binomial", "bernoulli", "normal"))
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--full", action="store_true", help="also time the site kernel (span stamps)")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)

    import torch
    from torch.distributions import Bernoulli, Binomial, NegativeBinomial, Normal, Poisson

    import bench
    import mininf_amd

    kind, p = args.likelihood, 32

    def workload(name, device, world, rank):
        gen = torch.Generator().manual_seed(0)
        n_total, n_obs = (1_000_000, 1_000_000) if name == "c3" else (10_000_000, 65536)
        X = torch.randn(n_total, p, generator=gen)
        X[:, 0] = 1.0   # the intercept is a column of X
        eta = X @ (0.1 * torch.randn(p, generator=gen))
        trials = 12.0
        if kind == "poisson":
            y = torch.poisson(eta.exp(), generator=gen)
        elif kind == "binomial":
            y = torch.binomial(torch.full_like(eta, trials), torch.sigmoid(eta), generator=gen)
        elif kind == "negative_binomial":
            y = torch.poisson(3.0 * torch.ones_like(eta), generator=gen)
        elif kind == "bernoulli":
            y = (torch.rand(n_total, generator=gen) < torch.sigmoid(eta)).float()
        else:
            y = eta + torch.randn(n_total, generator=gen)
        X, y = X.to(device), y.to(device)

        def model():
            theta = mininf_amd.sample("theta", Normal(0, 1), sample_shape=p)
            with mininf_amd.batch(n_total):
                with mininf_amd.no_log_prob():
                    Xs = mininf_amd.sample("X", Normal(0, 1), sample_shape=(n_total, p))
                if kind == "poisson":
                    mininf_amd.sample("y", Poisson((Xs @ theta).exp()))
                elif kind == "binomial":
                    mininf_amd.sample("y", Binomial(trials, logits=Xs @ theta))
                elif kind == "negative_binomial":
                    mininf_amd.sample("y", NegativeBinomial(trials, logits=Xs @ theta))
                elif kind == "bernoulli":
                    mininf_amd.sample("y", Bernoulli(logits=Xs @ theta))
                else:
                    mininf_amd.sample("y", Normal(Xs @ theta, 1))

        # a narrow guide: the predictors of all particles stay within a few units
        guide = mininf_amd.nn.ParameterizedDistribution(
            Normal, loc=1e-3 * torch.randn(p, generator=gen),
            scale=(-4.0 + 1e-3 * torch.randn(p, generator=gen)).exp()).to(device)
        if n_obs == n_total:
            static = mininf_amd.condition(model, X=X, y=y)

            def conditioned():
                return static
        else:
            loader = mininf_amd.DeviceDataLoader(X, y, batch_size=n_obs, shuffle=True,
                                                 drop_last=True, seed=0)

            def conditioned():
                Xb, yb = loader.next()
                return mininf_amd.condition(model, X=Xb, y=yb)

        k_local = args.particles
        return dict(
            desc=f"{name.upper()}-shaped {kind} regression, {n_total}x{p} (minibatch {n_obs}), "
                 f"MF Normal guide, {k_local} particles",
            k_local=k_local, n=n_obs, module=guide, guide=lambda: {"theta": guide()},
            conditioned=conditioned, evals=k_local * (n_obs + p), lr=0.001,
            dominant_N=n_obs, bound="mfma", flops_per_eval=4.0 * p, bytes_per_eval=0.0,
            kernel=f"the site launch of the {kind} likelihood", flop_note="2 x P FMA per eval",
            data=f"synthetic: X ~ N(0,1)[{n_total},{p}], y ~ {kind}(X theta*) (seed 0)")

    bench.workload = workload
    sys.argv = ["bench.py", "--gpus", "1", "--config", args.shape, "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-other-configs"] + \
        (["--full"] if args.full else []) + (["--eager"] if args.eager else [])
    bench.main()


if __name__ == "__main__":
    main()
