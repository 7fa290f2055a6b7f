"""
ms_per_step of a softmax (multinomial logistic) regression, Categorical(logits = X @ Theta) with
Theta [P, C], measured by bench.py's own run_config (graph replay, warm-up, timed replays):
bench.workload is replaced for the run, bench.py is not edited.

  python tools/softmax_regression_bench.py --shape c4
  MININF_AMD_DEFER_MATMUL=0 python tools/softmax_regression_bench.py --shape c4
  python tools/softmax_regression_bench.py --shape c4 --root ../parent-checkout

Shapes: c4 = 1e7 rows resident, DeviceDataLoader minibatches of 65536 (shuffled); c3 = whole data
per step, --rows of them (default 1e5: the materialised path holds two [K, N, C] tensors, 2 GB
there). P = 32, K = 256, C = 10 unless given. MININF_AMD_DEFER_MATMUL=0 is the materialised path of
the same tree (a [K, N, C] GEMM, mi_categorical_forward, a second GEMM); --root DIR imports bench.py
and the package from another checkout (e.g. the parent commit, which always materialises), so that
the builds can be run alternately in one session. Prints bench.py's JSON line (ms_per_step).
"""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("c3", "c4"), default="c4")
    ap.add_argument("--rows", type=int, default=100_000, help="rows of the c3 shape")
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--categories", type=int, default=10)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)

    import torch
    from torch.distributions import Categorical, Normal

    import bench
    import mininf_amd

    p, c = args.features, args.categories

    def workload(name, device, world, rank):
        gen = torch.Generator().manual_seed(0)
        n_total, n_obs = (args.rows, args.rows) if name == "c3" else (10_000_000, 65536)
        X = torch.randn(n_total, p, generator=gen)
        X[:, 0] = 1.0   # the intercept is a column of X
        eta = X @ (0.3 * torch.randn(p, c, generator=gen))
        y = torch.distributions.Categorical(logits=eta).sample()
        X, y = X.to(device), y.to(device)

        def model():
            theta = mininf_amd.sample("theta", Normal(0, 1), sample_shape=(p, c))
            with mininf_amd.batch(n_total):
                with mininf_amd.no_log_prob():
                    Xs = mininf_amd.sample("X", Normal(0, 1), sample_shape=(n_total, p))
                mininf_amd.sample("y", Categorical(logits=Xs @ theta))

        guide = mininf_amd.nn.ParameterizedDistribution(
            Normal, loc=1e-3 * torch.randn(p, c, generator=gen),
            scale=(-4.0 + 1e-3 * torch.randn(p, c, generator=gen)).exp()).to(device)
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
            desc=f"{name.upper()}-shaped softmax regression, {n_total}x{p}, {c} categories "
                 f"(minibatch {n_obs}), MF Normal guide, {k_local} particles",
            k_local=k_local, n=n_obs, module=guide, guide=lambda: {"theta": guide()},
            conditioned=conditioned, evals=k_local * (n_obs + p * c), lr=0.001,
            dominant_N=n_obs, bound="mfma", flops_per_eval=4.0 * p * c, bytes_per_eval=0.0,
            kernel="the site launch of the Categorical likelihood",
            flop_note="2 x P x C FMA per eval",
            data=f"synthetic: X ~ N(0,1)[{n_total},{p}], y ~ Categorical(X Theta*) (seed 0)")

    bench.workload = workload
    sys.argv = ["bench.py", "--gpus", "1", "--config", args.shape, "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-other-configs"] + \
        (["--eager"] if args.eager else [])
    bench.main()


if __name__ == "__main__":
    main()
