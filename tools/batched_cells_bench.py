"""What a batch of small periodic cells costs.  B = 64 structures of 8 atoms (the conventional cubic cell of
tools/small_cell_bench.py, every structure with its own slightly strained cell and its own displacements), hidden 32, l_max 2,
2 layers, envelope 6, energies + forces + stresses:
(a) ONE call of ``BatchedPeriodicEnergyModel`` (one selection of image rows, one open graph, one backward), against
(b) the loop a user had to write before: 64 calls of ``PeriodicEnergyModel(..., cell=, images=True)`` with the same weights.

Both legs include their graph builds.  The legs alternate inside one process after a warm-up; every repeat is timed with a host
clock around work that ends in a device synchronise (the loop is bound by the host's launches, which device events alone would
miss) and the medians are written to --out (default profiles/batched_cells_bench.json) and printed as one JSON line, with the
rows and edges of both and the agreement of the outputs.  The kernel launches of one call of each leg are counted afterwards
in a run of their own under the profiler (not timed).  No threshold: a record.

    python tools/batched_cells_bench.py [--structures B] [--repeats R] [--warmup W] [--out PATH]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402,F401
from scalable_e3_gnn_amd.batched import BatchedPeriodicEnergyModel, PeriodicEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.cell_images import batched_cell_image_graph  # noqa: E402

CELL = [[5.4, 0.0, 0.0], [0.0, 5.4, 0.0], [0.0, 0.0, 5.4]]
FRAC = [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]]
R_CUT = 5.0
HIDDEN, LAYERS, LMAX, ENVELOPE = 32, 2, 2, 6


def structures(B, seed=1):
    """-> cells [B,3,3] fp64, pos [8 B, 3] fp32, batch [8 B], x [8 B, 4] fp32: every structure strained by up to 2 % and
    displaced off the symmetric sites"""
    rng = np.random.default_rng(seed)
    cells, pos = [], []
    for _ in range(B):
        cell = np.asarray(CELL) @ (np.eye(3) + 0.02 * rng.uniform(-1, 1, (3, 3)))
        cells.append(cell)
        pos.append((np.asarray(FRAC, np.float64) + 0.01 * rng.standard_normal((len(FRAC), 3))) @ cell)
    n = len(FRAC)
    return (np.stack(cells), np.concatenate(pos).astype(np.float32), np.repeat(np.arange(B), n),
            rng.standard_normal((B * n, 4)).astype(np.float32))


def timed(legs, repeats, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):  # the legs alternate: drifts of clock / temperature hit both alike
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def count_launches(fn):
    """kernel launches of one call, from the profiler's device activity (a run of its own)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batched_cells_bench.json"))
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": forces need it
    dev = torch.device("cuda:0")
    B = args.structures
    cells, pos, batch, x = structures(B)
    torch.manual_seed(0)
    batched = BatchedPeriodicEnergyModel("1x0e+1x1o", HIDDEN, LAYERS, lmax=LMAX, envelope=ENVELOPE).to(dev).eval()
    single = PeriodicEnergyModel("1x0e+1x1o", HIDDEN, LAYERS, lmax=LMAX, envelope=ENVELOPE).to(dev).eval()
    single.load_state_dict(batched.state_dict())
    xd, pd, bd = torch.as_tensor(x).to(dev), torch.as_tensor(pos).to(dev), torch.as_tensor(batch).to(dev)
    cl = cells.tolist()
    n = len(FRAC)
    parts = [(xd[b * n:(b + 1) * n].contiguous(), pd[b * n:(b + 1) * n].contiguous(), cl[b]) for b in range(B)]
    legs = {"batched": lambda: batched(xd, pd, bd, R_CUT, cl, forces=True, stress=True),
            "loop": lambda: [single(xb, pb, R_CUT, cell=cb, forces=True, stress=True, images=True) for xb, pb, cb in parts]}
    (e_b, f_b, s_b), loop = legs["batched"](), legs["loop"]()
    e_l, f_l, s_l = torch.stack([o[0] for o in loop]), torch.cat([o[1] for o in loop]), torch.stack([o[2] for o in loop])
    images, split, _, _, _ = batched_cell_image_graph(pd, xd, bd, R_CUT, cl)
    med, every = timed(legs, args.repeats, args.warmup)
    out = {"model": {"lmax": LMAX, "hidden": HIDDEN, "layers": LAYERS, "envelope": ENVELOPE},
           "legs": "energies + forces + stresses, graph builds included; host clock around a device synchronise",
           "device": torch.cuda.get_device_name(0), "structures": B, "atoms_per_structure": n, "r": R_CUT,
           "shells": sorted({tuple(m) for m in images.shells}),
           "batched": {"rows": images.n_owned + images.n_ghost, "image_rows": images.n_ghost, "edges": split.graph.num_edges,
                       "dropped_edges": split.dropped},
           "agreement": {"energies": float((e_b - e_l).abs().max() / e_l.abs().max()),
                         "forces": float((f_b - f_l).abs().max() / f_l.abs().max()),
                         "stresses": float((s_b - s_l).abs().max() / s_l.abs().max())},
           "median_ms": med, "repeats_ms": every, "loop_ms_per_structure": round(med["loop"] / B, 4),
           "loop_over_batched": round(med["loop"] / med["batched"], 2), "launches": "not measured"}

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    write()                                                       # the times are on disk before the profiler starts
    try:
        out["launches"] = {k: count_launches(fn) for k, fn in legs.items()}
    except Exception as exc:                                      # the times stand without the counts
        out["launches"] = f"not measured: {type(exc).__name__}: {exc}"
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
