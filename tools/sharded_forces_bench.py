"""What forces cost on the sharded path.  (a) A world-1 periodic self-halo `ShardedEnergyModel(forces=True)` step against
(b) the `PeriodicEnergyModel(forces=True)` step on the same box: 100 k dyadic particles in the periodic unit box (k ~ 24
neighbours), l_max 2, H 32, 2 layers, fp32 -- the step of tools/stress_bench.py.  Both build their graph inside the step.
(c) The two kernels of the differentiable refresh at [n_local, 288] with the halo's own index lists against their torch
restatements: `e3_halo_refresh` vs `clone + index_copy_`, `e3_halo_reduce` vs `zero the ghost rows + index_add_`.

The legs alternate inside one process after a warm-up; every repeat is timed with device events and the medians are
printed as one JSON line (and written to --out).  World 1 exchanges nothing between ranks: the transport is not in (a).

    python tools/sharded_forces_bench.py [--particles N] [--repeats R] [--warmup W] [--out profiles/sharded_forces_bench.json]
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
from scalable_e3_gnn_amd import ShardedEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel  # noqa: E402
from scalable_e3_gnn_amd.sharding import (GridHalo, halo_reduce, halo_reduce_torch, halo_refresh,  # noqa: E402
                                          halo_refresh_torch)

BOX = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def cutoff(n, k=24.0):
    return float((3 * k / (4 * torch.pi * n)) ** (1 / 3))


def timed(legs, repeats, inner, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):  # the legs alternate: drifts of clock / temperature hit all alike
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": forces need it
    dev = torch.device("cuda:0")
    n, D = args.particles, 288
    gen = torch.Generator(device=dev).manual_seed(2)
    pos = torch.randint(0, 1 << 16, (n, 3), device=dev, generator=gen).float() / float(1 << 16)
    x = torch.randn(n, 4, device=dev, generator=gen)
    r = cutoff(n)
    torch.manual_seed(0)
    ref = PeriodicEnergyModel("1x0e+1x1o", 32, 2, lmax=2).to(dev).eval()
    sh = ShardedEnergyModel("1x0e+1x1o", 32, 2, 2).to(dev).eval()
    sh.load_state_dict(ref.state_dict())
    halo = GridHalo((1, 1, 1), *BOX, periodic=True)
    steps, steps_all = timed({"sharded_self_halo": lambda: sh(x, pos, r, halo, forces=True),
                              "periodic": lambda: ref(x, pos, r, *BOX, periodic=True, forces=True)}, args.repeats, 1, args.warmup)
    e_s, f_s = sh(x, pos, r, halo, forces=True)
    e_p, f_p = ref(x, pos, r, *BOX, periodic=True, forces=True)
    out = {"step": {"particles": n, "lmax": 2, "hidden": 32, "layers": 2, "r": round(r, 5),
                    "ghosts_per_owned": round(halo.ghost_fraction(), 4), "median_ms": steps, "repeats_ms": steps_all,
                    "sharded_over_periodic": round(steps["sharded_self_halo"] / steps["periodic"], 4),
                    "energy_rel_diff": float(abs(e_s - e_p) / abs(e_p)),
                    "forces_rel_diff": float((f_s - f_p).abs().max() / f_p.abs().max())}}
    # (c) the kernels alone, on the index lists the last step left in the halo
    slot, red_ptr, red_k = halo._maps()
    recv_idx, send_idx = halo._recv_idx, halo._send_idx
    n_local = slot.numel()
    h = torch.randn(n_local, D, device=dev, generator=gen)
    recv = torch.randn(halo.n_ghost, D, device=dev, generator=gen)
    back = torch.randn(send_idx.numel(), D, device=dev, generator=gen)
    assert torch.equal(halo_refresh(h, recv, slot, recv_idx), halo_refresh_torch(h, recv, recv_idx))
    kern, kern_all = timed({"e3_halo_refresh": lambda: halo_refresh(h, recv, slot, recv_idx),
                            "clone_index_copy": lambda: halo_refresh_torch(h, recv, recv_idx),
                            "e3_halo_reduce": lambda: halo_reduce(h, back, slot, red_ptr, red_k, recv_idx, send_idx),
                            "zero_index_add": lambda: halo_reduce_torch(h, back, recv_idx, send_idx)}, args.repeats, 20,
                           args.warmup)
    es = h.element_size()
    out["kernels"] = {"rows": n_local, "ghost_rows": halo.n_ghost, "sent_rows": int(send_idx.numel()), "D": D,
                      "median_ms": kern, "repeats_ms": kern_all,
                      "refresh_bytes": (2 * n_local) * D * es,   # every output row written, one source row read for it
                      "reduce_bytes": (2 * n_local - halo.n_ghost + int(send_idx.numel())) * D * es}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
