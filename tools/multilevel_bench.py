"""
ms_per_step of the multilevel regression (a varying intercept plus fixed effects), of the grouped
model of DESIGN section 0o or of the varying-slope models of section 0t, measured by bench.py's own run_config (graph replay of the whole step,
warm-up, timed replays): bench.workload is replaced for the run, bench.py is not edited.

  python tools/multilevel_bench.py --model multilevel        # y ~ Normal(alpha[g] + X theta, sigma),
                                                             # c ~ Poisson(exp(a + alpha[g] + X theta))
  python tools/multilevel_bench.py --model grouped           # y ~ Normal(alpha[g], sigma),
                                                             # c ~ Poisson(exp(a + b alpha[g]))
  python tools/multilevel_bench.py --model slopes            # y ~ Normal(alpha[g] + beta[g] x, sigma),
                                                             # c ~ Poisson(exp(a + alpha[g] + beta[g] x))
  python tools/multilevel_bench.py --model slopes --slopes 2 # two slopes and X theta in both sites

N = 1 000 000, G = 1000, P = 8, K = 256, mean-field Normal guides. Prints bench.py's JSON line
(ms_per_step, fusions). MININF_AMD_DEFER_SUM=0 (slopes: MININF_AMD_DEFER_SLOPE=0) gives the
materialised step; --root DIR imports
bench.py and the package from another checkout (e.g. the parent commit), so that the builds can be
run alternately in one session.
"""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("multilevel", "grouped", "slopes"), default="multilevel")
    ap.add_argument("--slopes", type=int, default=1, choices=(1, 2),
                    help="--model slopes: 1 slope and no X, or 2 slopes and X @ theta")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)

    import torch
    from torch.distributions import Normal, Poisson

    import bench
    import mininf_amd

    n, groups, p, multilevel = args.rows, args.groups, args.features, args.model == "multilevel"
    slopes = args.slopes if args.model == "slopes" else 0
    multilevel = multilevel or slopes == 2   # (fixed effects)

    def workload(name, device, world, rank):
        gen = torch.Generator().manual_seed(0)
        group = torch.randint(0, groups, (n,), generator=gen)
        alpha = 0.8 * torch.randn(groups, generator=gen)
        X = torch.randn(n, p, generator=gen)
        eta = alpha[group]
        if multilevel:
            eta = eta + X @ (0.2 * torch.randn(p, generator=gen))
        columns = [torch.randn(n, generator=gen) for _ in range(slopes)]
        for z in columns:
            eta = eta + (0.4 * torch.randn(groups, generator=gen))[group] * z
        columns = [z.to(device) for z in columns]
        y = eta + 0.5 * torch.randn(n, generator=gen)
        c = torch.poisson((0.3 + 0.6 * eta).exp(), generator=gen)
        group, X, y, c = group.to(device), X.to(device), y.to(device), c.to(device)

        def model():
            al = mininf_amd.sample("alpha", Normal(0, 1), sample_shape=(groups,))
            sigma = mininf_amd.sample("log_sigma", Normal(0, 1)).exp()
            a = mininf_amd.sample("a", Normal(0, 1))
            if slopes:
                eta = al[group]
                for s, z in enumerate(columns):
                    beta = mininf_amd.sample(f"beta{s}", Normal(0, 1), sample_shape=(groups,))
                    eta = eta + beta[group] * z
                if multilevel:
                    eta = eta + X @ mininf_amd.sample("theta", Normal(0, 1), sample_shape=(p,))
                mininf_amd.sample("y", Normal(eta, sigma))
                mininf_amd.sample("c", Poisson((a + eta).exp()))
            elif multilevel:
                theta = mininf_amd.sample("theta", Normal(0, 1), sample_shape=(p,))
                mininf_amd.sample("y", Normal(al[group] + X @ theta, sigma))
                mininf_amd.sample("c", Poisson((a + al[group] + X @ theta).exp()))
            else:
                b = mininf_amd.sample("b", Normal(0, 1))
                mininf_amd.sample("y", Normal(al[group], sigma))
                mininf_amd.sample("c", Poisson((a + b * al[group]).exp()))

        shapes = {"alpha": (groups,), "log_sigma": (), "a": ()}
        shapes.update({"theta": (p,)} if multilevel else {} if slopes else {"b": ()})
        shapes.update({f"beta{s}": (groups,) for s in range(slopes)})
        # narrow guides: the predictors of all particles stay within a few units
        guides = torch.nn.ModuleDict({
            key: mininf_amd.nn.ParameterizedDistribution(
                Normal, loc=1e-2 * torch.randn(shape, generator=gen),
                scale=(-3.0 + 1e-2 * torch.randn(shape, generator=gen)).exp())
            for key, shape in shapes.items()}).to(device)
        static = mininf_amd.condition(model, y=y, c=c)
        k_local = args.particles
        return dict(
            desc=f"{args.model} model, N {n}, G {groups}, P {p if multilevel else 0}, "
                 f"S {slopes}, MF Normal "
                 f"guides, {k_local} particles",
            k_local=k_local, n=n, module=guides,
            guide=lambda: {key: g() for key, g in guides.items()},
            conditioned=lambda: static, evals=2 * k_local * n, lr=0.001,
            dominant_N=n, bound="valu", flops_per_eval=4.0 * p, bytes_per_eval=0.0,
            kernel="the gathered site launches", flop_note="2 x P FMA per eval",
            data=f"synthetic: group ~ U[0,{groups}), X ~ N(0,1)[{n},{p}] (seed 0)")

    bench.workload = workload
    sys.argv = ["bench.py", "--gpus", "1", "--config", "c3", "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-other-configs"]
    bench.main()


if __name__ == "__main__":
    main()
