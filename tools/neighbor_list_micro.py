"""What a Verlet list saves per step.  The bench's cloud -- 1 M uniform particles in the unit box, r = cutoff(n) of bench.py
(k ~ 24), open box -- with skin = 0.25 r and every particle displaced by a random 0.2 skin since the build:

    radius_graph  : radius_graph(pos, r, lo, hi) plus g.dst -- what a step pays without a list (the yardstick)
    update        : NeighborList.update(pos) while the list holds (gather + displacement, count, scan, fill, one host read)
    rebuild       : NeighborList.update(pos) on a step that rebuilds (the builder at r + skin, then the same update)

The legs alternate in one process after a warm-up; every repeat is timed with device events and, around the same calls,
with the host clock up to the synchronisation (an update ends in a host read, the builder holds two).  Medians go out as
one JSON line with the spread of the yardstick, the ratios and the bytes an update has to move.  A second block times a
10 k-atom periodic ``forces=True`` step of PeriodicEnergyModel on one trajectory with and without ``neighbors=``.  Kernel
times: run under `rocprofv3 --kernel-trace --stats` (separately from this timing; `--repeats 3 --inner 1 --no-model`
keeps the trace short).

    python tools/neighbor_list_micro.py [--particles N] [--skin-ratio S] [--repeats R] [--inner I] [--warmup W] [--no-model]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import models  # noqa: E402,F401
from bench import cutoff  # noqa: E402
from scalable_e3_gnn_amd import NeighborList  # noqa: E402
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.radius_graph import radius_graph  # noqa: E402


def timed(legs, repeats, inner, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(repeats):  # the legs alternate: drifts of clock / temperature hit all alike
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            host[k].append((time.perf_counter() - t0) * 1e3 / inner)
            dev[k].append(a.elapsed_time(b) / inner)
    return dev, host


def graph_legs(args, dev):
    n = args.particles
    r = cutoff(n)
    skin = args.skin_ratio * r
    lo, hi = [0.0] * 3, [1.0] * 3
    gen = torch.Generator(device=dev).manual_seed(0)
    pos0 = torch.rand(n, 3, device=dev, generator=gen)
    u = torch.randn(n, 3, device=dev, generator=gen)
    pos = (pos0 + 0.2 * skin * u / u.norm(dim=1, keepdim=True)).contiguous()
    nl = NeighborList(r, skin, lo, hi)
    nl.update(pos0)
    stored_edges = nl.stored.num_edges

    def fresh():
        return radius_graph(pos, r, lo, hi).dst

    def update():
        g = nl.update(pos)
        assert not nl.rebuilt
        return g

    def rebuild():
        nl.invalidate()
        nl.update(pos0)  # built where it was: the update leg keeps its displacements

    # the pruned graph is the fresh one (pairs in caller ids), checked once outside the timing
    g, want = update(), radius_graph(pos, r, lo, hi)
    code = lambda q: torch.sort(q.perm.long()[q.dst.long()] * n + q.perm.long()[q.src.long()]).values  # noqa: E731
    same = g.num_edges == want.num_edges and bool(torch.equal(code(g), code(want)))
    info = {"particles": n, "r": r, "skin": skin, "edges_stored": stored_edges, "edges_r": g.num_edges,
            "pairs_equal_fresh_graph": same,
            "update_bytes_needed": stored_edges * 4 + g.num_edges * 8 + n * 60}
    return {"radius_graph": fresh, "update": update, "rebuild": rebuild}, info


def model_step(args, dev):
    """A 10 k-atom periodic forces=True step on one drifting trajectory, alternating with / without neighbors=."""
    n = args.model_particles
    r = cutoff(n)
    skin = args.skin_ratio * r
    lo, hi = [0.0] * 3, [1.0] * 3
    gen = torch.Generator(device=dev).manual_seed(1)
    pos = torch.rand(n, 3, device=dev, generator=gen)
    u = torch.randn(n, 3, device=dev, generator=gen)
    u = 0.05 * skin * u / u.norm(dim=1, keepdim=True)
    x = torch.randn(n, 4, device=dev, generator=gen)
    torch.manual_seed(2)
    model = PeriodicEnergyModel("1x0e+1x1o", args.hidden, args.layers, lmax=2).to(dev).eval()
    nl = NeighborList(r, skin, lo, hi, True)
    t = {"neighbors": [], "fresh_graph": []}
    worst = 0.0
    for k in range(args.model_steps + 2):
        p = (pos + k * u).contiguous()
        out = {}
        for name, kw in (("neighbors", dict(neighbors=nl)), ("fresh_graph", dict(lo=lo, hi=hi))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = model(x, p, r, forces=True, **kw)
            torch.cuda.synchronize()
            if k >= 2 and not (name == "neighbors" and nl.rebuilt):  # two warm-up steps; rebuild steps are counted apart
                t[name].append((time.perf_counter() - t0) * 1e3)
        f0, f1 = out["neighbors"][1], out["fresh_graph"][1]
        worst = max(worst, float((f0 - f1).abs().max() / f1.abs().max()))
    return {"particles": n, "r": r, "skin": skin, "hidden": args.hidden, "layers": args.layers, "steps": args.model_steps,
            "builds": nl.builds, "step_ms": {k: round(statistics.median(v), 3) for k, v in t.items()},
            "forces_max_rel_diff": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--skin-ratio", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model-particles", type=int, default=10_000)
    ap.add_argument("--model-steps", type=int, default=12)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    legs, info = graph_legs(args, dev)
    d, h = timed(legs, args.repeats, args.inner, args.warmup)
    med = {k: round(statistics.median(v), 4) for k, v in d.items()}
    med_host = {k: round(statistics.median(v), 4) for k, v in h.items()}
    yard = d["radius_graph"]
    line = dict(info, median_ms=med, median_host_ms=med_host, repeats_ms={k: [round(t, 4) for t in v] for k, v in d.items()},
                radius_graph_spread_ms=round(max(yard) - min(yard), 4),
                radius_graph_over_update=round(med["radius_graph"] / med["update"], 3),
                rebuild_over_radius_graph=round(med["rebuild"] / med["radius_graph"], 3),
                update_GB_per_s=round(info["update_bytes_needed"] / med["update"] * 1e-6, 1))
    if not args.no_model:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what forces= uses
            line["model_step"] = model_step(args, dev)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
