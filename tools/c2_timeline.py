"""
Where C2's site kernel (k_site_bcast_smem, the matrix instantiation) spends its time, per workgroup:
a build of bcast_site.hip with MI_SITES_TIMELINE defined, in which thread 0 of every workgroup stamps
the constant-rate clock (s_memrealtime, 100 MHz) at entry, after the per-particle logits, after the
chunk pass and its barrier round, after the first matrix pass, after the matrix loop, after the
chunks' values are stored and at exit (the MI_TL points of bcast_site.hip).
`run` replays the C2 bench step (24 steps per graph replay, as bench.py), then one more replay with
the rows cleared, and prints the phase statistics of the last launch of that replay -- by dispatch
rank on the CU (block b is the b / 256-th workgroup of its CU), for the particle-constant
workgroups (chunk groups 0-3) and for the side job -- and which workgroups leave last.
MININF_AMD_BCAST_CPW selects the chunks per workgroup as in any build.

    python tools/c2_timeline.py build [name]   (on the CPU: tools/_variants/<name, c2tl>/)
    MININF_AMD_LIB=tools/_variants/c2tl/libmininf_amd.so python tools/c2_timeline.py run [out.json]
"""
import ctypes
import json
import os
import sys

import numpy as np
import torch
from torch.distributions import Bernoulli, Beta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mininf_amd as mi  # noqa: E402
from mininf_amd import _native as nat  # noqa: E402
from mininf_amd.graph import StepGraph  # noqa: E402


def build_variant(name="c2tl"):
    """The timeline build of the tree's bcast_site.hip, through tools/variant_build.py."""
    import subprocess
    import tempfile
    src = open(os.path.join(ROOT, "mininf_amd", "csrc", "bcast_site.hip")).read()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bcast_site.hip")
        open(path, "w").write("#define MI_SITES_TIMELINE 1\n" + src)
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "variant_build.py"), name,
                        f"bcast_site.hip={path}"], check=True)


def main():
    dev = torch.device("cuda:0")
    n, K = 1_000_000, 4096
    x = (torch.rand(n, generator=torch.Generator().manual_seed(0)) < 0.7).float().to(dev)

    def model():
        theta = mi.sample("theta", Beta(2, 2))
        mi.sample("x", Bernoulli(theta), sample_shape=[n])

    guide = mi.nn.ParameterizedDistribution(Beta, concentration0=2.0, concentration1=2.0).to(dev)
    cond = mi.condition(model, x=x)
    loss_fn = mi.nn.EvidenceLowerBoundLoss(num_particles=K, seed=3)
    opt = mi.optim.Adam(guide.parameters(), lr=0.02)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(cond, {"theta": guide()})
        loss.backward()
        opt.step()
        return loss

    lib = nat.lib()
    lib.mi_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    graph = StepGraph(step, warmup=2, repeat=24)
    for _ in range(40):   # ~40 ms of device time: clocks up
        graph()
    torch.cuda.synchronize()
    assert lib.mi_debug_timeline_clear() == 0
    graph()
    torch.cuda.synchronize()
    raw = np.zeros(8192 * 8, dtype=np.uint64)
    assert lib.mi_debug_timeline(raw.ctypes.data, raw.nbytes) == 0
    rows = raw.reshape(-1, 8).astype(np.int64)
    block = np.nonzero(rows[:, 0] > 0)[0]           # blockIdx.x of every workgroup that ran
    rows = rows[block]
    kind, kblock, group = rows[:, 7] % 2, (rows[:, 7] // 2) % 16, rows[:, 7] // 32
    base = rows[:, 0].min()
    t = (rows[:, :7] - base) / 100.0                # us since the first workgroup's entry
    main_wg, side = kind == 0, kind == 1

    def stats(v):
        if v.size == 0:
            return None
        return [round(float(q), 2) for q in (np.min(v), np.percentile(v, 10), np.median(v),
                                              np.percentile(v, 90), np.max(v))]

    def phases(sel):
        m = t[sel]
        return {"n": int(sel.sum()), "entry": stats(m[:, 0]), "logits": stats(m[:, 1] - m[:, 0]),
                "chunk pass + barrier": stats(m[:, 2] - m[:, 1]),
                "first matrix pass": stats(m[:, 3] - m[:, 2]),
                "later matrix passes": stats(m[:, 4] - m[:, 3]),
                "value sums + stores": stats(m[:, 5] - m[:, 4]),
                "slot rows, constant segment, flags": stats(m[:, 6] - m[:, 5]),
                "exit": stats(m[:, 6])}
    out = {"cpw": os.environ.get("MININF_AMD_BCAST_CPW", "auto"),
           "workgroups": int(main_wg.sum()), "side_workgroups": int(side.sum()),
           "kernel_span_us": round(float(t[:, 6].max()), 2),
           "columns": "min / p10 / median / p90 / max (us)",
           "all main workgroups": phases(main_wg),
           "by dispatch rank (blockIdx.x // 256)": {
               int(q): phases(main_wg & (block // 256 == q)) for q in np.unique(block[main_wg] // 256)},
           "particle-constant workgroups (chunk groups 0-3)": phases(main_wg & (group < 4)),
           "other main workgroups": phases(main_wg & (group >= 4))}
    if side.any():
        out["side job"] = {"n": int(side.sum()), "entry": stats(t[side, 0]), "exit": stats(t[side, 6])}
    last = np.argsort(-t[:, 6])[:8]
    out["last 8 to exit: (blockIdx.x, side job, chunk group, particle block, entry, exit)"] = [
        (int(block[i]), int(kind[i]), int(group[i]), int(kblock[i]), round(float(t[i, 0]), 2),
         round(float(t[i, 6]), 2)) for i in last]
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    if sys.argv[1:2] == ["build"]:
        build_variant(*sys.argv[2:3])
    else:
        main()
