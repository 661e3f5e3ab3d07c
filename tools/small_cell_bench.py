"""What a small periodic cell costs.  Energy + forces + stress of a PeriodicEnergyModel (l_max 2, H 16, 2 layers, envelope 6)
(a) through the image rows of the cell itself (``images=True``: open graph over [particles | lattice images]) and (b) through
the existing minimum-image path on the smallest supercell with 2 r < every perpendicular height, built by hand -- what a user
had to do before.  Cases: a 2-atom fcc-like primitive cell and an 8-atom cubic cell at a cutoff near the cell size.

Both legs include their graph build.  The legs alternate inside one process after a warm-up; every repeat is timed with device
events and the medians are written to --out (default profiles/small_cell_bench.json) and printed as one JSON line, with the
rows, the kept edges and the dropped edges of both: the open build over the extended cloud also forms the edges INTO image
rows, which ``split_graph`` then drops -- that share is recorded, cutting it is a separate job.  No threshold: a record.

    python tools/small_cell_bench.py [--repeats R] [--warmup W] [--out PATH]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402,F401
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.cell_images import cell_image_graph  # noqa: E402
from scalable_e3_gnn_amd.radius_graph import cell_params, radius_graph  # noqa: E402

CASES = {   # name -> (cell rows, fractional positions, r)
    "fcc_primitive_2": ([[0.0, 2.7, 2.7], [2.7, 0.0, 2.7], [2.7, 2.7, 0.0]], [[0.0, 0.0, 0.0], [0.25, 0.25, 0.25]], 5.0),
    "cubic_8": ([[5.4, 0.0, 0.0], [0.0, 5.4, 0.0], [0.0, 0.0, 5.4]],
                [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                 [.75, .75, .25]], 5.0),
}


def smallest_supercell(cell, r):
    """k_a = the fewest repeats with 2 r < k_a h_a"""
    heights = cell_params(cell)[2]
    return tuple(int(np.floor(2.0 * r / h)) + 1 for h in heights)


def timed(legs, repeats, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):  # the legs alternate: drifts of clock / temperature hit both alike
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def run_case(name, model, dev, repeats, warmup):
    cell, frac, r = CASES[name]
    cell_np = np.asarray(cell, np.float64)
    rng = np.random.default_rng(1)
    pos = (np.asarray(frac, np.float64) + 0.01 * rng.standard_normal((len(frac), 3))) @ cell_np   # off the symmetric sites
    x = rng.standard_normal((len(pos), 4)).astype(np.float32)
    tile = smallest_supercell(cell, r)
    offs = [np.asarray(n, np.float64) @ cell_np for n in itertools.product(*(range(k) for k in tile))]
    pos_s = np.concatenate([pos + o for o in offs])
    cell_s = (cell_np * np.asarray(tile, np.float64)[:, None]).tolist()
    xd, pd = torch.as_tensor(x).to(dev), torch.as_tensor(pos.astype(np.float32)).to(dev)
    xs, ps = xd.repeat(len(offs), 1), torch.as_tensor(pos_s.astype(np.float32)).to(dev)
    legs = {"images": lambda: model(xd, pd, r, cell=cell, forces=True, stress=True, images=True),
            "supercell": lambda: model(xs, ps, r, cell=cell_s, forces=True, stress=True)}
    (e_i, f_i, s_i), (e_s, f_s, s_s) = legs["images"](), legs["supercell"]()
    images, split, _, _ = cell_image_graph(pd, xd, r, cell)
    g = radius_graph(ps, r, cell=cell_s)
    med, every = timed(legs, repeats, warmup)
    kept = split.graph.num_edges
    return {"cell": cell, "particles": len(pos), "r": r, "shells": list(images.shells), "supercell": list(tile),
            "images": {"rows": images.n_owned + images.n_ghost, "image_rows": images.n_ghost, "edges": kept,
                       "dropped_edges": split.dropped, "dropped_share": round(split.dropped / max(1, kept + split.dropped), 4)},
            "supercell_path": {"rows": len(pos_s), "edges": g.num_edges, "dropped_edges": 0},
            "agreement": {"energy_per_cell": abs(float(e_i) - float(e_s) / len(offs)) / max(1.0, abs(float(e_i))),
                          "forces": float((f_i - f_s[:len(pos)]).abs().max() / f_i.abs().max()),
                          "stress": float((s_i - s_s).abs().max() / s_i.abs().max())},
            "median_ms": med, "repeats_ms": every, "images_over_supercell": round(med["images"] / med["supercell"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "small_cell_bench.json"))
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": forces need it
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = PeriodicEnergyModel("1x0e+1x1o", 16, 2, lmax=2, envelope=6).to(dev).eval()
    out = {"model": {"lmax": 2, "hidden": 16, "layers": 2, "envelope": 6}, "legs": "energy + forces + stress, graph build included",
           "device": torch.cuda.get_device_name(0),
           "cases": {name: run_case(name, model, dev, args.repeats, args.warmup) for name in CASES}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
