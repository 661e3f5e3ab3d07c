"""What the migration pack costs next to the rebuild it precedes, on one MI355X at world 1 (a periodic self-halo).  The
bench's cloud -- 1 M uniform particles in the unit box -- with the row table of a driver that keeps pos, x[4], vel and an
int64 id per particle (W = 12 words) and a synthetic owner array that sends 1 % of the rows to each of four other ranks:

    pack        : e3_migrate_count, the one host read of the counts, e3_migrate_fill (sharding.migrate_rows)
    restatement : sharding.migrate_rows_torch on the device, on the same input -- the yardstick for the kernel
    build       : leg (d) of tools/sharded_list_micro.py in the same process: halo.setup + radius_graph + renumber +
                  split_graph at r, the rebuild every migration precedes -- the yardstick for the feature

The legs alternate in one process after a warm-up; every repeat is timed with device events and, around the same calls,
with the host clock up to the synchronisation.  Medians, the spread of each leg, the two ratios and the bytes the pack has
to move (from the shapes) go out as one JSON line, and to ``--out`` when given.

    python tools/migration_micro.py [--particles N] [--leave-percent P] [--repeats R] [--inner I] [--warmup W] [--out FILE]
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
from scalable_e3_gnn_amd.sharding import migrate_rows, migrate_rows_torch, pack_rows  # noqa: E402
from tools.neighbor_list_micro import timed  # noqa: E402
from tools.sharded_list_micro import legs_of  # noqa: E402

OTHERS = 4


def legs_and_info(args, dev):
    n, world = args.particles, OTHERS + 1
    gen = torch.Generator(device=dev).manual_seed(1)
    pos = torch.rand(n, 3, device=dev, generator=gen)
    x, vel = torch.randn(n, 4, device=dev, generator=gen), torch.randn(n, 3, device=dev, generator=gen)
    table, _ = pack_rows(pos, x, vel, torch.arange(n, device=dev))
    u = torch.rand(n, device=dev, generator=gen)
    share = args.leave_percent / 100.0
    owner = torch.clamp((u / share).floor().long() + 1, max=world).remainder(world).to(torch.int32)   # 0 = stays

    def pack():
        return migrate_rows(table, owner, 0, world)

    def restatement():
        return migrate_rows_torch(table, owner, 0, world)

    a, b = pack(), restatement()
    same = all(torch.equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
    sharded, sinfo = legs_of(argparse.Namespace(particles=n, skin_ratio=args.skin_ratio), dev)
    W = table.shape[1]
    n_leave = int(a[1].shape[0])
    info = {"particles": n, "row_words": W, "ranks": world, "rows_leaving": n_leave, "pack_equals_restatement": bool(same),
            "rebuild_local_rows": sinfo["local_rows"], "rebuild_edges": sinfo["edges_kept"],
            # from the shapes: owner read twice (count, fill), the table read once and written once, the block counts
            "pack_bytes_needed": 2 * 4 * n + 2 * 4 * n * W}
    return {"pack": pack, "restatement": restatement, "build": sharded["build"]}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--leave-percent", type=float, default=1.0, help="share of the rows sent to EACH of the four other ranks")
    ap.add_argument("--skin-ratio", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    legs, info = legs_and_info(args, dev)
    d, h = timed(legs, args.repeats, args.inner, args.warmup)
    med = {k: round(statistics.median(v), 4) for k, v in d.items()}
    line = dict(info, median_ms=med, median_host_ms={k: round(statistics.median(v), 4) for k, v in h.items()},
                spread_ms={k: round(max(v) - min(v), 4) for k, v in d.items()},
                repeats_ms={k: [round(t, 4) for t in v] for k, v in d.items()},
                restatement_over_pack=round(med["restatement"] / med["pack"], 3),
                pack_over_build=round(med["pack"] / med["build"], 4),
                pack_GB_per_s=round(info["pack_bytes_needed"] / med["pack"] * 1e-6, 1))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
