"""Periodic box on one GPU, two ways: (a) the periodic radius graph + SEGNN forward, against (b) the world-1 self-halo of
``GridHalo((1, 1, 1), ..., periodic=True)``: ``setup`` (wrap + ghost images, all 26 entries served by local copies) + the
local OPEN graph over ``[owned | ghost images]`` + ``split_graph`` + the overlapped forward.  1 M = 2^20 dyadic particles in
the unit box (k ~ 24 neighbours), l_max 2, H 32, 4 layers, fp32.

Also times the image selection alone on the same GPU tensors: the HIP pair (csrc/e3_halo.hip) against the torch
restatement ``select_images_torch`` (and checks that they agree bit for bit).  The legs alternate inside one process after a
warm-up, each repeat timed with device events; the medians go into one JSON line.

    python tools/periodic_shard_bench.py [--particles N] [--repeats R] [--steps K] [--warmup W]
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
from scalable_e3_gnn_amd.radius_graph import radius_graph  # noqa: E402
from scalable_e3_gnn_amd.segnn import SEGNN  # noqa: E402
from scalable_e3_gnn_amd.sharding import GridHalo, select_images, select_images_torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.particles
    r = float((3 * 24.0 / (4 * torch.pi * n)) ** (1 / 3))
    gen = torch.Generator(device=dev).manual_seed(1234)
    pos = torch.randint(0, 1 << 16, (n, 3), device=dev, generator=gen).float() / float(1 << 16)   # dyadic
    x = torch.randn(n, 4, device=dev, generator=gen)
    torch.manual_seed(0)
    model = SEGNN("1x0e+1x1o", args.hidden, "1x1o", args.layers, lmax=2).to(dev)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    state = {}

    def whole():
        g = radius_graph(pos, r, lo, hi, periodic=True)
        with torch.no_grad():
            out = model(x[g.perm.long()], g)
        state["E_whole"] = g.num_edges
        return out

    def self_halo():
        halo = GridHalo((1, 1, 1), lo, hi, periodic=True)
        lpos, lx = halo.setup(pos, x, r)
        g = radius_graph(lpos, r, [-2 * r] * 3, [1 + 2 * r] * 3)
        halo.renumber(g.perm)
        split = halo.split_graph(g)
        with torch.no_grad():
            out = model(lx[g.perm.long()], g, halo=halo, split=split)
        state["ghost_fraction"] = halo.ghost_fraction()
        state["E_local"] = g.num_edges
        state["E_kept"] = split.graph.num_edges
        return out

    sel = GridHalo((1, 1, 1), lo, hi, periodic=True)._selection(r)
    a, b = select_images(pos, lo, hi, True, r, sel), select_images_torch(pos, lo, hi, True, r, sel)
    assert a[2] == b[2] and all(torch.equal(u, v) for u, v in ((a[0], b[0]), (a[1], b[1]), (a[3], b[3])))
    del a, b
    legs = {"a_periodic_graph": whole, "b_self_halo": self_halo,
            "select_hip": lambda: select_images(pos, lo, hi, True, r, sel),
            "select_torch": lambda: select_images_torch(pos, lo, hi, True, r, sel),
            "setup": lambda: GridHalo((1, 1, 1), lo, hi, periodic=True).setup(pos, x, r)}
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
                out = step()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / args.steps)
            if k in ("a_periodic_graph", "b_self_halo"):
                assert torch.isfinite(out.float()).all()
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"particles": n, "r": r, "layers": args.layers, "hidden": args.hidden, "lmax": 2, "dtype": "fp32",
           "repeats": args.repeats, "steps_per_repeat": args.steps, "ghost_fraction": round(state["ghost_fraction"], 4),
           "E_whole": state["E_whole"], "E_local": state["E_local"], "E_kept": state["E_kept"],
           "ms": {k: round(v, 3) for k, v in med.items()},
           "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           "self_halo_over_periodic_graph": round(med["b_self_halo"] / med["a_periodic_graph"], 4),
           "select_torch_over_hip": round(med["select_torch"] / med["select_hip"], 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
