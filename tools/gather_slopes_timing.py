"""
Kernel-level times of mi_gather_slopes_forward (csrc/gather_linear_site.hip) through the C ABI, beside
mi_gather_linear_forward (P >= 1) or mi_gather_site_forward (P = 0) on the same rows without the
slope terms and beside the step's arithmetic as torch does it on the materialised predictor ([K, N]
gathers and products, the density, and autograd's scatter-adds).

  python tools/gather_slopes_timing.py [--n 1000000] [--groups 1000] [--particles 256] [--reps 20]

S in {1, 2, 4} at P in {0, 8}, Normal and Poisson. Each line is the median over --reps launches
(device events around one call: the site kernel and its finishing launches), after 3 warm-up calls.
Prints one JSON line per variant.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()

    import torch
    from torch.distributions import Normal, Poisson

    from mininf_amd import _native as nat

    N, G, K = args.n, args.groups, args.particles
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    index = torch.randint(0, G, (N,), generator=gen)
    sorted_group, order = torch.sort(index, stable=True)
    order, sorted_group = order.int().to(device), sorted_group.int().to(device)
    index = index.to(device)
    table = (0.3 * torch.randn(K, G, generator=gen)).to(device)
    betas = [(0.1 * torch.randn(K, G, generator=gen)).to(device) for _ in range(4)]
    columns = [torch.randn(N, generator=gen).to(device) for _ in range(4)]
    sigma = (0.5 + torch.rand(K, generator=gen)).to(device)
    X = torch.randn(N, 8, generator=gen).to(device)
    theta = (0.05 * torch.randn(K, 8, generator=gen)).to(device)
    values = {"normal": torch.randn(N, generator=gen).to(device),
              "poisson": torch.poisson(2 * torch.ones(N), generator=gen).to(device)}
    lib = nat.lib()
    stream = nat.stream_handle(device)

    def describe(family, P, S):
        M = nat.GatherSlopes()
        L = M.linear.site
        L.K, L.N, L.G = K, N, G
        L.family = nat.NORMAL if family == "normal" else nat.POISSON
        L.role[0].kind = nat.GATHER_GATHER
        L.role[0].link = nat.GATHER_LINK_EXP if family == "poisson" else nat.GATHER_LINK_IDENTITY
        L.role[0].data = table.data_ptr()
        L.role[0].stride_k, L.role[0].stride_g = table.stride()
        if family == "normal":
            L.role[1].kind = nat.GATHER_PARTICLE
            L.role[1].data = sigma.data_ptr()
            L.role[1].stride_k = 1
        L.order, L.sorted_group = order.data_ptr(), sorted_group.data_ptr()
        L.value = values[family].data_ptr()
        L.value_stride_i = 1
        L.value_kind = nat.GATHER_VALUE_FLOAT32
        L.grad_scale, L.site_scale = -1.0 / K, 1.0
        if P:
            M.linear.P = P
            M.linear.x, M.linear.theta = X.data_ptr(), theta.data_ptr()
            M.linear.x_stride_i, M.linear.x_stride_j = X.stride()
            M.linear.theta_stride_k, M.linear.theta_stride_j = theta.stride()
        M.S = S
        for s in range(S):
            M.slope[s].table = betas[s].data_ptr()
            M.slope[s].stride_k, M.slope[s].stride_g = betas[s].stride()
            M.slope[s].z = columns[s].data_ptr()
            M.slope[s].z_stride_i = 1
        return M

    def timed(call):
        for _ in range(3):
            call()
        times = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        return statistics.median(times), min(times), max(times)

    total = torch.empty(K, device=device)
    flags = torch.zeros(1, dtype=torch.int32, device=device)
    dtable = torch.empty(K, G, device=device)
    dsigma = torch.empty(K, device=device)
    dtheta = torch.empty(K, 8, device=device)
    dbetas = [torch.empty(K, G, device=device) for _ in range(4)]
    dslope = (nat.c_vp * nat.GATHER_MAX_SLOPES)(*(t.data_ptr() for t in dbetas))
    grads = nat.GatherGrads()
    grads.role[0], grads.role[1] = dtable.data_ptr(), dsigma.data_ptr()
    size = ctypes.c_size_t()

    def report(variant, family, P, S, ms):
        print(json.dumps({"variant": variant, "family": family, "N": N, "G": G, "K": K, "P": P,
                          "S": S, "median_ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
                          "max_ms": round(ms[2], 4), "reps": args.reps}), flush=True)

    for family in ("normal", "poisson"):
        for P in (0, 8):
            M = describe(family, P, 1)
            if P:
                nat.check(lib.mi_gather_linear_workspace_bytes(ctypes.byref(M.linear),
                                                               ctypes.byref(size)), "size")
                work = torch.empty(size.value, dtype=torch.uint8, device=device)
                report("mi_gather_linear_forward", family, P, 0, timed(lambda: nat.check(
                    lib.mi_gather_linear_forward(ctypes.byref(M.linear), work.data_ptr(), size.value,
                                                 total.data_ptr(), ctypes.byref(grads),
                                                 dtheta.data_ptr(), flags.data_ptr(), stream),
                    "forward")))
            else:
                nat.check(lib.mi_gather_site_workspace_bytes(ctypes.byref(M.linear.site),
                                                             ctypes.byref(size)), "size")
                work = torch.empty(size.value, dtype=torch.uint8, device=device)
                report("mi_gather_site_forward", family, 0, 0, timed(lambda: nat.check(
                    lib.mi_gather_site_forward(ctypes.byref(M.linear.site), work.data_ptr(),
                                               size.value, total.data_ptr(), ctypes.byref(grads),
                                               flags.data_ptr(), stream), "forward")))
            for S in (1, 2, 4):
                M = describe(family, P, S)
                nat.check(lib.mi_gather_slopes_workspace_bytes(ctypes.byref(M), ctypes.byref(size)),
                          "size")
                work = torch.empty(size.value, dtype=torch.uint8, device=device)
                report("mi_gather_slopes_forward", family, P, S, timed(lambda: nat.check(
                    lib.mi_gather_slopes_forward(ctypes.byref(M), work.data_ptr(), size.value,
                                                 total.data_ptr(), ctypes.byref(grads),
                                                 dtheta.data_ptr(), dslope, flags.data_ptr(),
                                                 stream), "forward")))
                assert int(flags.cpu()[0]) == 0

    # the same arithmetic through torch on the materialised [K, N] predictor
    for family in ("normal", "poisson"):
        for P, S in ((0, 1), (8, 2)):
            leaves = [t.clone().requires_grad_() for t in [table, *betas[:S]]]
            if P:
                leaves.append(theta.clone().requires_grad_())

            def step():
                eta = leaves[0][:, index]
                for s in range(S):
                    eta = eta + leaves[1 + s][:, index] * columns[s]
                if P:
                    eta = eta + leaves[-1] @ X.t()
                dist = Normal(eta, sigma[:, None], validate_args=False) if family == "normal" else \
                    Poisson(eta.exp(), validate_args=False)
                loss = dist.log_prob(values[family]).sum() * (-1.0 / K)
                torch.autograd.grad(loss, leaves)
            report("torch, materialised", family, P, S, timed(step))


if __name__ == "__main__":
    main()
