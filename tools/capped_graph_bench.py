"""What the neighbour cap costs and saves: graph build and a 4-layer l_max = 2, hidden-32 inference forward, uncapped against
radius_graph(..., max_neighbors=k).

  leg a  the bench cloud (1 M uniform points in the unit box, ~23.5 neighbours), uncapped vs k = 64.  Nothing is truncated
         there, so the difference is what the capped fill (e3_rg_cap_rowptr + e3_rg_fill_nearest) costs on its plain path.
  leg b  a clustered cloud (200 k points: eight blobs of sigma 0.01 plus a quarter uniform background -- the `clustered`
         generator of tests/test_radius_graph.py -- at r = 0.006, about a thousand neighbours at a blob's centre and
         neighbourhoods of several candidate chunks), uncapped vs k = 32: the edge count and everything proportional to it.

Build and forward are timed separately with device events after a warm-up; the variants of a leg alternate inside every
repeat, and the median over the repeats is reported with the spread (min, max).  There is no pass threshold.  Writes
profiles/capped_graph_bench.json and prints the same JSON.

    python tools/capped_graph_bench.py [--repeats R] [--warmup W] [--legs a,b] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import models  # noqa: E402,F401
from scalable_e3_gnn_amd.radius_graph import radius_graph  # noqa: E402
from scalable_e3_gnn_amd.segnn import SEGNN  # noqa: E402


def clustered(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(8, 3, generator=g)
    p = c[torch.randint(0, 8, (n,), generator=g)] + 0.01 * torch.randn(n, 3, generator=g)
    p[: n // 4] = torch.rand(n // 4, 3, generator=g)
    return p.clamp(0, 0.999999).float().to(dev)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return out, t0.elapsed_time(t1)


def run_leg(pos, x, r, caps, model, repeats, warmup):
    def build(k):
        return radius_graph(pos, r, [0, 0, 0], [1, 1, 1], max_neighbors=k)

    def forward(g):
        with torch.no_grad():
            return model(x[g.perm.long()], g)

    for k in caps:
        for _ in range(warmup):
            forward(build(k))
    torch.cuda.synchronize()
    tb, tf, graphs = {k: [] for k in caps}, {k: [] for k in caps}, {}
    for _ in range(repeats):
        for k in caps:   # the variants alternate: drifts of clock / temperature hit both alike
            g, ms = timed(lambda: build(k))
            tb[k].append(ms)
            out, ms = timed(lambda: forward(g))
            tf[k].append(ms)
            assert torch.isfinite(out).all()
            graphs[k] = g
    res = {}
    for k in caps:
        g = graphs[k]
        res["uncapped" if k is None else f"k{k}"] = {
            "E": g.num_edges, "full_edges": g.full_edges, "truncated": g.truncated,
            "build_ms": round(statistics.median(tb[k]), 3), "build_spread_ms": [round(min(tb[k]), 3), round(max(tb[k]), 3)],
            "forward_ms": round(statistics.median(tf[k]), 3),
            "forward_spread_ms": [round(min(tf[k]), 3), round(max(tf[k]), 3)]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "capped_graph_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SEGNN("1x0e+1x1o", 32, "1x1o", 4, lmax=2).to(dev)
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                check=True).stdout.strip()
    except Exception:
        commit = None
    res = {"device": torch.cuda.get_device_name(0), "parent_commit": commit, "layers": 4, "hidden": 32, "lmax": 2,
           "repeats": args.repeats, "warmup": args.warmup, "legs": {}}
    gen = torch.Generator(device=dev).manual_seed(1234)
    if "a" in args.legs.split(","):
        n = 1_000_000
        pos = torch.rand(n, 3, device=dev, generator=gen)
        x = torch.randn(n, 4, device=dev, generator=gen)
        r = float((3 * 24.0 / (4 * torch.pi * n)) ** (1 / 3))
        leg = run_leg(pos, x, r, (None, 64), model, args.repeats, args.warmup)
        assert leg["k64"]["truncated"] == 0 and leg["k64"]["E"] == leg["uncapped"]["E"]
        lo, hi = leg["uncapped"]["build_spread_ms"]
        leg["k64_build_minus_uncapped_ms"] = round(leg["k64"]["build_ms"] - leg["uncapped"]["build_ms"], 3)
        leg["uncapped_build_spread_ms"] = round(hi - lo, 3)
        res["legs"]["a_uniform_1m"] = {"particles": n, "r": r, **leg}
    if "b" in args.legs.split(","):
        n = 200_000
        pos = clustered(n, 3, dev)
        x = torch.randn(n, 4, device=dev, generator=gen)
        leg = run_leg(pos, x, 0.006, (None, 32), model, args.repeats, args.warmup)
        leg["edges_ratio"] = round(leg["k32"]["E"] / leg["uncapped"]["E"], 4)
        leg["forward_ratio"] = round(leg["k32"]["forward_ms"] / leg["uncapped"]["forward_ms"], 4)
        leg["build_ratio"] = round(leg["k32"]["build_ms"] / leg["uncapped"]["build_ms"], 4)
        res["legs"]["b_clustered_200k"] = {"particles": n, "r": 0.006, **leg}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
