"""
Kernel-level times of mi_gather_linear_forward (csrc/gather_linear_site.hip) through the C ABI, beside
mi_gather_site_forward on the same rows without the linear term and beside the step's arithmetic as
torch does it on the materialised predictor (a [K, N] product, a [K, N] gather, the density, and
autograd's second product and scatter-add).

  python tools/gather_linear_timing.py [--n 1000000] [--groups 1000] [--particles 256] [--reps 20]

Each line is the median over --reps launches (device events around one call: the site kernel and its
finishing launches), after 3 warm-up calls. Prints one JSON line per variant.
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
    ap.add_argument("--torch-p", type=int, default=8, help="P of the materialised torch variant")
    args = ap.parse_args()

    import torch
    from mininf_amd import _native as nat

    N, G, K = args.n, args.groups, args.particles
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    index = torch.randint(0, G, (N,), generator=gen)
    sorted_group, order = torch.sort(index, stable=True)
    order, sorted_group = order.int().to(device), sorted_group.int().to(device)
    index = index.to(device)
    table = (0.3 * torch.randn(K, G, generator=gen)).to(device)
    sigma = (0.5 + torch.rand(K, generator=gen)).to(device)
    X32 = torch.randn(N, 32, generator=gen).to(device)
    theta32 = (0.05 * torch.randn(K, 32, generator=gen)).to(device)
    values = {"normal": torch.randn(N, generator=gen).to(device),
              "poisson": torch.poisson(2 * torch.ones(N), generator=gen).to(device)}
    lib = nat.lib()
    stream = nat.stream_handle(device)

    def site(family):
        L = nat.GatherSite()
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
        return L

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
    grads = nat.GatherGrads()
    grads.role[0], grads.role[1] = dtable.data_ptr(), dsigma.data_ptr()
    size = ctypes.c_size_t()

    def report(variant, family, P, ms):
        print(json.dumps({"variant": variant, "family": family, "N": N, "G": G, "K": K, "P": P,
                          "median_ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
                          "max_ms": round(ms[2], 4), "reps": args.reps}), flush=True)

    for family in ("normal", "poisson"):
        L = site(family)
        nat.check(lib.mi_gather_site_workspace_bytes(ctypes.byref(L), ctypes.byref(size)), "size")
        work = torch.empty(size.value, dtype=torch.uint8, device=device)
        report("mi_gather_site_forward", family, 0, timed(lambda: nat.check(
            lib.mi_gather_site_forward(ctypes.byref(L), work.data_ptr(), size.value,
                                       total.data_ptr(), ctypes.byref(grads), flags.data_ptr(),
                                       stream), "forward")))
        for P in (8, 16, 32):
            X = X32[:, :P].contiguous()
            theta = theta32[:, :P].contiguous()
            dtheta = torch.empty(K, P, device=device)
            M = nat.GatherLinear()
            M.site = L
            M.P = P
            M.x, M.theta = X.data_ptr(), theta.data_ptr()
            M.x_stride_i, M.x_stride_j = X.stride()
            M.theta_stride_k, M.theta_stride_j = theta.stride()
            nat.check(lib.mi_gather_linear_workspace_bytes(ctypes.byref(M), ctypes.byref(size)),
                      "size")
            work = torch.empty(size.value, dtype=torch.uint8, device=device)
            report("mi_gather_linear_forward", family, P, timed(lambda: nat.check(
                lib.mi_gather_linear_forward(ctypes.byref(M), work.data_ptr(), size.value,
                                             total.data_ptr(), ctypes.byref(grads),
                                             dtheta.data_ptr(), flags.data_ptr(), stream),
                "forward")))
            assert int(flags.cpu()[0]) == 0

    # the same arithmetic through torch on the materialised [K, N] predictor
    from torch.distributions import Normal, Poisson
    P = args.torch_p
    X = X32[:, :P].contiguous()
    for family in ("normal", "poisson"):
        leaves = [table.clone().requires_grad_(), theta32[:, :P].clone().requires_grad_()]

        def step():
            eta = leaves[0][:, index] + leaves[1] @ X.t()
            dist = Normal(eta, sigma[:, None], validate_args=False) if family == "normal" else \
                Poisson(eta.exp(), validate_args=False)
            loss = dist.log_prob(values[family]).sum() * (-1.0 / K)
            torch.autograd.grad(loss, leaves)
        report("torch, materialised", family, P, timed(step))


if __name__ == "__main__":
    main()
