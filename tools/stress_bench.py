"""What the virial costs.  (a) The geometry backward alone at 1 M dyadic particles in the periodic unit box (k ~ 24
neighbours), l_max 2, random upstream gradients: e3_edge_geometry_backward_pbc against e3_edge_geometry_backward_strained
with one structure (S = 1, the store-and-sum reduction) and with 64 structures (S = 64, atomics per row).  (b) A
100 k-particle PeriodicEnergyModel step (l_max 2, H 32, 2 layers): energy + forces against energy + forces + stress.

The legs alternate inside one process after a warm-up; every repeat is timed with device events and the medians are
printed as one JSON line.  Kernel times: run under `rocprofv3 --kernel-trace --stats` (separately from this timing).

    python tools/stress_bench.py [--particles N] [--step-particles M] [--repeats R] [--inner K] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import models  # noqa: E402,F401
from scalable_e3_gnn_amd import _lib  # noqa: E402
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.radius_graph import radius_graph  # noqa: E402


def cutoff(n, k=24.0):
    return float((3 * k / (4 * torch.pi * n)) ** (1 / 3))


def dyadic(n, gen, dev):
    return torch.randint(0, 1 << 16, (n, 3), device=dev, generator=gen).float() / float(1 << 16)


def timed(legs, repeats, inner, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):  # the legs alternate: drifts of clock / temperature hit both alike
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def backward_legs(n, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    g = radius_graph(dyadic(n, gen, dev), cutoff(n), [0, 0, 0], [1, 1, 1], periodic=True)
    E, lmax, ny = g.num_edges, 2, 9
    gY = torch.randn(E, ny, device=dev, generator=gen)
    gd = torch.randn(E, device=dev, generator=gen)
    gA = torch.randn(n, ny, device=dev, generator=gen)
    gpos = torch.empty(n, 3, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.e3_edge_geometry_backward_strained_workspace_bytes(n), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    common = (g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), n, lmax)
    grads = (gY.data_ptr(), gd.data_ptr(), gA.data_ptr(), gpos.data_ptr())

    def plain():
        _lib.check(lib.e3_edge_geometry_backward_pbc(*common, g.box_arg, *grads, stream))

    def strained(S):
        eps = torch.zeros(S, 3, 3, device=dev)
        sid = torch.randint(0, S, (n,), device=dev, generator=gen, dtype=torch.int32) if S > 1 else None
        gs = torch.empty(S, 3, 3, device=dev)

        def run():
            _lib.check(lib.e3_edge_geometry_backward_strained(
                *common, g.box_arg, eps.data_ptr(), sid.data_ptr() if sid is not None else None, S, *grads,
                gs.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return run

    return {"plain": plain, "strained_S1": strained(1), "strained_S64": strained(64)}, E


def step_legs(n, dev):
    gen = torch.Generator(device=dev).manual_seed(2)
    pos = dyadic(n, gen, dev)
    x = torch.randn(n, 4, device=dev, generator=gen)
    torch.manual_seed(0)
    model = PeriodicEnergyModel("1x0e+1x1o", 32, 2, lmax=2).to(dev).eval()
    r = cutoff(n)
    box = ([0, 0, 0], [1, 1, 1])
    return {"energy_forces": lambda: model(x, pos, r, *box, forces=True),
            "energy_forces_stress": lambda: model(x, pos, r, *box, forces=True, stress=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--step-particles", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": the step below needs it
    dev = torch.device("cuda:0")
    legs, E = backward_legs(args.particles, dev)
    bwd, bwd_all = timed(legs, args.repeats, args.inner, args.warmup)
    out = {"backward": {"particles": args.particles, "edges": E, "lmax": 2, "median_ms": bwd, "repeats_ms": bwd_all,
                        "strained_S1_over_plain": round(bwd["strained_S1"] / bwd["plain"], 4)}}
    del legs
    torch.cuda.empty_cache()
    if not args.skip_step:
        steps, steps_all = timed(step_legs(args.step_particles, dev), args.repeats, 1, args.warmup)
        out["step"] = {"particles": args.step_particles, "lmax": 2, "hidden": 32, "layers": 2, "median_ms": steps,
                       "repeats_ms": steps_all,
                       "stress_over_forces": round(steps["energy_forces_stress"] / steps["energy_forces"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
