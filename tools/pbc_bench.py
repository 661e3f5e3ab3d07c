"""Open vs periodic box vs general cell at the bench configuration: graph build + SEGNN forward per step, 1 M uniform
particles at unit density (k ~ 24 neighbours), l_max 2, H 32, 4 layers, fp32 and bf16 storage.

The legs alternate inside one process after a warm-up, each repeat timed with device events:
  open      the unit box, no periodicity
  periodic  the unit box, periodic=True (the orthorhombic kernels)
  cube      the same unit cube given as cell= (the cell kernels on the same points; must give the periodic edge count)
  cell      T = rows (1,0,0), (0.25,0.875,0), (0.125,-0.25,0.75) scaled to unit volume, uniform fractional coordinates
The periodic graphs have more edges than the open one (no face deficit), so the comparison is per edge.  Prints one JSON
line.  Kernel times (rg_scan_kernel, msg_ws_kernel per launch): one run of their own under the profiler, one repeat:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/pbc_bench.py --repeats 1 --warmup 1

    python tools/pbc_bench.py [--particles N] [--repeats R] [--steps K] [--warmup W] [--legs open,periodic,cube,cell]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--legs", default="open,periodic,cube,cell")
    args = ap.parse_args()
    kinds = args.legs.split(",")
    assert kinds and all(k in ("open", "periodic", "cube", "cell") for k in kinds), args.legs
    dev = torch.device("cuda:0")
    n = args.particles
    r = float((3 * 24.0 / (4 * torch.pi * n)) ** (1 / 3))
    gen = torch.Generator(device=dev).manual_seed(1234)
    pos = torch.rand(n, 3, device=dev, generator=gen)
    x = torch.randn(n, 4, device=dev, generator=gen)
    cube = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    scale = 0.65625 ** (-1.0 / 3.0)  # |det T| = 0.65625
    tcell = [[scale * v for v in row] for row in ((1.0, 0.0, 0.0), (0.25, 0.875, 0.0), (0.125, -0.25, 0.75))]
    pos_t = pos @ torch.tensor(tcell, device=dev)  # uniform fractional coordinates: unit density as in the box
    torch.manual_seed(0)
    model32 = SEGNN("1x0e+1x1o", args.hidden, "1x1o", args.layers, lmax=2).to(dev)
    model16 = SEGNN("1x0e+1x1o", args.hidden, "1x1o", args.layers, lmax=2).to(dev).bfloat16()
    legs = {}
    for dtype, model in (("fp32", model32), ("bf16", model16)):
        xd = x if dtype == "fp32" else x.bfloat16()
        for kind in kinds:
            def step(model=model, xd=xd, kind=kind):
                if kind == "cube":
                    g = radius_graph(pos, r, cell=cube)
                elif kind == "cell":
                    g = radius_graph(pos_t, r, cell=tcell)
                else:
                    g = radius_graph(pos, r, [0, 0, 0], [1, 1, 1], periodic=kind == "periodic")
                with torch.no_grad():
                    out = model(xd[g.perm.long()], g)
                return g, out
            legs[(dtype, kind)] = step
    for step in legs.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    edges = {}
    for _ in range(args.repeats):  # the legs alternate: drifts of clock / temperature hit both alike
        for k, step in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                g, out = step()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / args.steps)
            edges[k] = g.num_edges
            assert torch.isfinite(out.float()).all()
    res = {"particles": n, "r": r, "layers": args.layers, "hidden": args.hidden, "lmax": 2, "repeats": args.repeats,
           "steps_per_repeat": args.steps, "legs": {}}
    for (dtype, kind), ts in times.items():
        med = statistics.median(ts)
        E = edges[(dtype, kind)]
        res["legs"][f"{dtype}_{kind}"] = {
            "E": E, "ms_per_step": round(med, 3), "particles_per_s": round(n / (med * 1e-3)),
            "ms_per_million_edges": round(med / (E / 1e6), 4),
            "spread_ms": [round(min(ts), 3), round(max(ts), 3)]}
    for dtype in ("fp32", "bf16"):
        per_edge = {k: res["legs"][f"{dtype}_{k}"]["ms_per_million_edges"] for k in kinds}
        if "cube" in kinds and "periodic" in kinds:  # the same points, the same lattice: the same graph
            assert edges[(dtype, "cube")] == edges[(dtype, "periodic")], (edges[(dtype, "cube")], edges[(dtype, "periodic")])
        for k, base in (("periodic", "open"), ("cube", "periodic"), ("cell", "periodic")):
            if k in kinds and base in kinds:
                res[f"{dtype}_{k}_over_{base}_per_edge"] = round(per_edge[k] / per_edge[base], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
