"""Equal-count Morton key ranges on one GPU: what one rank of eight pays for its ghost selection.  A clustered cloud of
``8 x particles`` (unit cube, 60 % of it in a blob at (0.3, 0.65, 0.6), sigma 0.15; k ~ 24 neighbours on average) is cut into
``world = 8`` key ranges (``MortonPartition.fit``, no process group), and rank ``self_rank = 3`` selects the ghosts of its
~``particles`` = 2^20 owned particles for the seven others: the HIP pair (csrc/e3_morton_halo.hip: count + one host read +
fill) against the torch restatement ``select_morton_torch`` on the same GPU tensors -- what the layout would cost without
the kernel -- after checking that they agree bit for bit.  ``fit`` of the rank's own share (keys + histogram + splitters) is
timed beside them.  The legs alternate inside one process after a warm-up, each repeat timed with device events; the
medians go into one JSON line.  Kernel times: run the same script under ``rocprofv3 --kernel-trace --stats``.

    python tools/morton_shard_bench.py [--particles N] [--repeats R] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import models  # noqa: E402,F401
from scalable_e3_gnn_amd.sharding import MortonPartition, select_morton, select_morton_torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20, help="per rank; the cloud has world times as many")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--self-rank", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    world, me = args.world, args.self_rank
    n = args.particles * world
    r = float((3 * 24.0 / (4 * torch.pi * n)) ** (1 / 3))
    gen = torch.Generator(device=dev).manual_seed(1234)
    pos = torch.rand(n, 3, device=dev, generator=gen)
    blob = torch.rand(n, device=dev, generator=gen) < 0.6
    centre = torch.tensor([0.3, 0.65, 0.6], device=dev)
    pos = torch.where(blob[:, None], centre + 0.15 * torch.randn(n, 3, device=dev, generator=gen), pos)
    pos.clamp_(0.0, 1.0 - 2.0 ** -20)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    part = MortonPartition(lo, hi, r, world).fit(pos)
    assert all(abs(c - n / world) < part.hist_max for c in part.counts)
    own = pos[part.owner_of(pos) == me].contiguous()
    del pos, blob
    sel = (own, part.lo, part.hi, part.grid, r, part.splitters, me)
    a, b = select_morton(*sel), select_morton_torch(*sel)
    assert a[1] == b[1] and torch.equal(a[0], b[0]), "HIP selection differs from the torch restatement"
    ghosts = a[1]
    del a, b
    legs = {"select_hip": lambda: select_morton(*sel), "select_torch": lambda: select_morton_torch(*sel),
            "fit_own_share": lambda: MortonPartition(lo, hi, r, world).fit(own)}
    for step in legs.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.repeats):  # the legs alternate: drifts of clock / temperature hit both alike
        for k, step in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                step()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / args.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"particles_per_rank": args.particles, "cloud": n, "world": world, "self_rank": me, "r": r, "grid": list(part.grid),
           "fullest_cell": part.hist_max, "owned": part.counts, "selected_from": int(own.shape[0]), "ghosts_sent": ghosts,
           "peers": [q for q, c in enumerate(ghosts) if c], "ghosts_over_owned": round(sum(ghosts) / max(1, own.shape[0]), 4),
           "repeats": args.repeats, "steps_per_repeat": args.steps,
           "ms": {k: round(v, 4) for k, v in med.items()},
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "select_torch_over_hip": round(med["select_torch"] / med["select_hip"], 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
