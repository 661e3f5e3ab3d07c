"""What the sharded Verlet list saves per step, on one MI355X at world 1 (a periodic self-halo: every entry is a local copy).
The bench's cloud -- 1 M uniform particles in the unit box, r = cutoff(n) of bench.py (k ~ 24) -- with skin = 0.25 r and every
particle displaced by a random 0.2 skin since the build:

    fused       : e3_nl_update_split on the stored graph, then the one host read of its stats
    composition : e3_nl_update, a host read (the pruned count), e3_split_edges on its result, a host read (the three counts)
                  -- the yardstick for the kernel
    update      : ShardedNeighborList.update(pos, x) while the list holds (displacement, the shared word, positions and
                  features along the stored entries, the fused entry, one host read)
    build       : halo.setup + radius_graph + renumber + split_graph at r -- what a sharded step pays without a list (the
                  yardstick for the feature)

The legs alternate in one process after a warm-up; every repeat is timed with device events and, around the same calls,
with the host clock up to the synchronisation.  Medians, the spread of each leg, the two ratios and the bytes each leg has
to move (from the shapes) go out as one JSON line, and to ``--out`` when given.

    python tools/sharded_list_micro.py [--particles N] [--skin-ratio S] [--repeats R] [--inner I] [--warmup W] [--out FILE]
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
from bench import cutoff  # noqa: E402
from scalable_e3_gnn_amd import ShardedNeighborList, _lib  # noqa: E402
from scalable_e3_gnn_amd.radius_graph import radius_graph  # noqa: E402
from scalable_e3_gnn_amd.sharding import GridHalo  # noqa: E402
from tools.neighbor_list_micro import timed  # noqa: E402


def legs_of(args, dev):
    n = args.particles
    r = cutoff(n)
    skin = args.skin_ratio * r
    lo, hi = [0.0] * 3, [1.0] * 3
    gen = torch.Generator(device=dev).manual_seed(0)
    pos0 = torch.rand(n, 3, device=dev, generator=gen)
    u = torch.randn(n, 3, device=dev, generator=gen)
    pos = (pos0 + 0.2 * skin * u / u.norm(dim=1, keepdim=True)).contiguous()
    x = torch.randn(n, 4, device=dev, generator=gen)
    halo = GridHalo((1, 1, 1), lo, hi, periodic=True)
    nl = ShardedNeighborList(r, skin, halo)
    nl.update(pos0, x)
    g = nl.stored.graph
    N, E = g.perm.numel(), g.num_edges
    ghost8 = nl._ghost8
    lpos = halo.update_positions(pos)[0].contiguous()
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    i32 = dict(dtype=torch.int32, device=dev)
    pos4 = torch.empty((N, 4), device=dev)
    rowptr, rowptr2 = torch.empty(N + 1, **i32), torch.empty(N + 1, **i32)
    outs = [torch.empty(max(E, 1), **i32) for _ in range(8)]
    stats, counts = torch.zeros(4, **i32), torch.zeros(4, **i32)
    ws_f = torch.empty(int(lib.e3_nl_update_split_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    ws_n = torch.empty(int(lib.e3_nl_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    ws_s = torch.empty(int(lib.e3_split_edges_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    head = (lpos.data_ptr(), g.perm.data_ptr(), g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr())

    def fused():
        _lib.check(lib.e3_nl_update_split(*head, ghost8.data_ptr(), N, E, r, pos4.data_ptr(), rowptr.data_ptr(),
                                          *[o.data_ptr() for o in outs[:6]], stats.data_ptr(), ws_f.data_ptr(), stream))
        return stats.tolist()

    def composition():
        _lib.check(lib.e3_nl_update(*head, N, E, r, pos4.data_ptr(), rowptr.data_ptr(), outs[6].data_ptr(), outs[7].data_ptr(),
                                    stats.data_ptr(), ws_n.data_ptr(), stream))
        _, e_r = stats[:2].tolist()
        _lib.check(lib.e3_split_edges(rowptr.data_ptr(), outs[6].data_ptr(), ghost8.data_ptr(), N, e_r, rowptr2.data_ptr(),
                                      *[o.data_ptr() for o in outs[:6]], counts.data_ptr(), ws_s.data_ptr(), stream))
        return counts.tolist()

    def update():
        c = nl.update(pos, x)
        assert not nl.rebuilt
        return c

    def build():
        h = GridHalo((1, 1, 1), lo, hi, periodic=True)
        lp, _ = h.setup(pos, x, r)
        gg = radius_graph(lp, r, *h.local_bounds(r))
        h.renumber(gg.perm)
        return h.split_graph(gg)

    # outside the timing: the two kernel legs agree, and the list's graph is the fresh one's size
    _, ek, ei, eb = fused()
    kept = [o[:c].clone() for o, c in zip(outs[:6], (ek, ek, ei, ei, eb, eb))]
    ck, ci, cb, _ = composition()
    same = (ek, ei, eb) == (ck, ci, cb) and all(torch.equal(a, o[:a.numel()]) for a, o in zip(kept, outs[:6]))
    e_all = int(stats[1])                                       # e3_nl_update's count: the ghost rows' edges included
    fresh = build()
    info = {"particles": n, "local_rows": N, "ghost_rows": N - n, "r": r, "skin": skin, "edges_stored": E,
            "edges_kept": ek, "edges_interior": ei, "edges_boundary": eb, "fused_equals_composition": bool(same),
            "kept_equals_fresh_build": fresh.graph.num_edges == ek,
            # past the cache, from the shapes: both walk the stored src twice (count, fill) and gather / write the node
            # arrays (perm 4, pos 12, ref 16, pos4 16 written and read, two rowptr 8, counts and offsets);
            # fused: + three lists of (src, dst); composition: + its pruned list written, read twice by the split, and
            # the split's three lists
            "fused_bytes_needed": 2 * 4 * E + 16 * ek + N * 92,
            "composition_bytes_needed": 2 * 4 * E + 8 * e_all + 2 * 4 * e_all + 16 * ek + N * 116}
    return {"fused": fused, "composition": composition, "update": update, "build": build}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--skin-ratio", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    legs, info = legs_of(args, dev)
    d, h = timed(legs, args.repeats, args.inner, args.warmup)
    med = {k: round(statistics.median(v), 4) for k, v in d.items()}
    line = dict(info, median_ms=med, median_host_ms={k: round(statistics.median(v), 4) for k, v in h.items()},
                spread_ms={k: round(max(v) - min(v), 4) for k, v in d.items()},
                repeats_ms={k: [round(t, 4) for t in v] for k, v in d.items()},
                composition_over_fused=round(med["composition"] / med["fused"], 3),
                build_over_update=round(med["build"] / med["update"], 3),
                fused_GB_per_s=round(info["fused_bytes_needed"] / med["fused"] * 1e-6, 1))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
