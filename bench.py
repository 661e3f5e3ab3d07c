#!/usr/bin/env python3
"""bench.py — radius-graph build + SEGNN forward on N MI355X (one process per GPU).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one synthetic batch already resident in HBM:
    Morton sort + cell scan (CSR radius graph)  ->  edge geometry  ->  SEGNN forward (L layers)
Rank 0 prints ONE JSON line: `value` (particles/s over all ranks), `ms_per_step` (wall time of one timed step), `metric`,
`unit`, `higher_is_better`, `dtype`.  A plain run does only what that line needs: set-up, warm-up, the timed steps and, with
`--dump-outputs DIR`, the last timed step's outputs.  With `--full` the line also carries the figures that cost runs or
instrumentation of their own:
  roofline     : the dominant kernel (largest total time among the timed launches: the fused message kernel), timed
                 live with HIP events on the launch stream; achieved = algorithmic flops (x3 for the fp16 split) or bytes
                 / avg launch time; traffic = HBM bytes per launch from committed rocprofv3 --pmc passes (traffic_source)
  cpu_baseline : the CPU oracle pipeline (reference op pattern for every TP) on a bounded sample after a warm-up,
                 all host cores, rank 0, N=1 only; cpu_baseline_best_effort: the best CPU formulation we know.
  bf16_storage : a second timed leg of the same workload in bf16 storage (l_max = 2, fp32 runs only).
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import numpy as np
import torch

METRIC = "particles/sec (octree build + SEGNN fwd), 1M pts l_max=2, 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F32_PEAK_TF = 157.3   # MI355X_MICROARCH.md: fp32-input MFMA (v_mfma_f32_32x32x2_f32) dense peak
MFMA_BF16_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: bf16 MFMA dense peak (~2.5 PF)
DUMP_BYTES = 64 << 20      # --dump-outputs: at most this much in all


def cutoff(n, k=24.0):
    return float((3.0 * k / (4.0 * math.pi * n)) ** (1.0 / 3.0))


def cpu_baseline(args, state):
    """CPU pipelines on `--cpu-sample` particles at the same neighbour density, after an untimed warm-up pass:
    (1) "port": the oracle pipeline with the reference's op pattern for every tensor product (the reported baseline);
    (2) "best_effort": the same arithmetic in the best CPU formulation we know (contiguous slices, GEMM on raw channels,
        einsum with the coupling) -- SURVEY.md §8d asks for it so that no ratio is quoted against a strawman."""
    from oracle import graph_oracle as G
    from oracle import segnn_oracle as S

    n = args.cpu_sample
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(avail, 16))  # the GPU box's CPU share for one GPU is 16 cores
    torch.set_num_threads(cores)
    params = {k: v.detach().float().cpu().numpy() for k, v in state.items()}  # CPU baseline always runs in fp32
    io = ("1x0e+1x1o", "1x1o")

    def port(*a):
        if args.lmax == 1:
            return S.forward_torch_cpu(params, args.hidden, args.layers, *io, *a)
        return S.forward_l2_torch_cpu(params, args.hidden, args.layers, *io, *a)

    def best(*a):
        return S.forward_l2_torch_cpu(params, args.hidden, args.layers, *io, *a, fast=True, lmax=args.lmax)

    def run(fn, npts):
        pos = torch.rand(npts, 3, generator=torch.Generator().manual_seed(0)).numpy()
        x = torch.randn(npts, 4, generator=torch.Generator().manual_seed(1)).numpy()
        t0 = time.perf_counter()
        perm, rowptr, src = G.graph(pos, [0, 0, 0], [1, 1, 1], cutoff(npts))
        with torch.no_grad():
            fn(x[perm], pos[perm], rowptr, src)
        return time.perf_counter() - t0, len(src)

    run(port, 1000)  # warm-up: library initialisation, thread pool, first-touch allocations
    run(best, 1000)
    dt, E = run(port, n)
    dtb, _ = run(best, n)
    desc = (f"{n} particles, same density (k~24, E={E}), lmax={args.lmax} {args.layers} layers H={args.hidden} fp32; "
            f"C cell-list graph (1 thread) + torch-CPU SEGNN ({cores} threads); one timed pass after a 1000-particle warm-up")
    return ({"value": n / dt, "unit": "particles/s", "cores": cores, "kind": "port", "seconds": dt,
             "sample": desc + "; every tensor product in the reference's op pattern (gather -> products -> cat -> matmul -> "
                              "column scatter -> norm, its l<=2 generalisation when lmax=2)"},
            {"value": n / dtb, "unit": "particles/s", "cores": cores, "kind": "best_effort", "seconds": dtb,
             "sample": desc + "; best-effort CPU formulation (contiguous slices, GEMM on raw channels, einsum with the coupling)"})


def spawn_ranks(n):
    """One child process per rank (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as torch.distributed.run would set them);
    rank 0's JSON line goes to this process's stdout.  Returns the worst child return code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def roofline_of(dom_tag, dom, traffic_file):
    """roofline object of one timed kernel (profiling.summary() entry)."""
    sec = dom["avg_ms"] * 1e-3
    gbs = dom["bytes_per_launch"] / sec / 1e9
    tfs = dom["flops_per_launch"] / sec / 1e12
    split = "x3 split" in dom["kernel"]          # fp32 products as 3 f16 MFMA products (hi*hi + hi*lo + lo*hi)
    native16 = "bf16 storage" in dom["kernel"]
    mfma_peak = MFMA_BF16_PEAK_TF if (split or native16) else MFMA_F32_PEAK_TF
    exec_mult = 3.0 if split else 1.0
    mfma_bound = dom["flops_per_launch"] * exec_mult / (mfma_peak * 1e12) > dom["bytes_per_launch"] / (HBM_PEAK_GBS * 1e9)
    roof = {"bound": "mfma" if mfma_bound else "hbm", "kernel": dom["kernel"] + "  [" + dom_tag + "]",
            "achieved": tfs * exec_mult if mfma_bound else gbs, "peak": mfma_peak if mfma_bound else HBM_PEAK_GBS,
            "unit": "TFLOP/s" if mfma_bound else "GB/s",
            "frac": (tfs * exec_mult / mfma_peak) if mfma_bound else (gbs / HBM_PEAK_GBS), "traffic": None,
            "mfma_mode": ("fp16x3 split: one fp32 product = 3 f16 MFMA products (hi*hi + hi*lo + lo*hi), fp32 accumulate; "
                          "`achieved` = 3 x algorithmic flops / time" if split else
                          "bf16 operands, fp32 accumulate" if native16 else "fp32"),
            "frac_on_hbm_roof": gbs / HBM_PEAK_GBS, "frac_on_mfma_roof": tfs * exec_mult / mfma_peak,
            "avg_launch_ms": dom["avg_ms"], "launches": dom["launches"],
            "algorithmic_bytes_per_launch": dom["bytes_per_launch"],
            "algorithmic_flops_per_launch": dom["flops_per_launch"],
            "algorithmic_GBps": gbs, "algorithmic_TFLOPps": tfs,
            # what the matrix pipe really executes per launch (the dst half of product #1 is contracted once per node by the
            # pre-mix launch, not per edge): `frac` above prices the ALGORITHMIC flops, this field the issued MFMAs
            "executed_flops_per_launch": dom.get("executed_flops_per_launch", dom["flops_per_launch"]),
            "frac_executed_on_mfma_roof": dom.get("executed_flops_per_launch", dom["flops_per_launch"]) * exec_mult / sec / 1e12 / mfma_peak}
    if traffic_file and os.path.exists(traffic_file):
        t = json.load(open(traffic_file))
        roof["traffic"] = t.get("hbm_bytes_per_launch")
        roof["traffic_source"] = {k: t.get(k) for k in ("file", "commit", "command", "kernel", "fetch_bytes_per_launch",
                                                        "write_bytes_per_launch", "note")}
        roof["traffic_source"]["file"] = os.path.relpath(traffic_file, REPO)
    return roof


def dump_outputs(outdir, g, out):
    """The last timed step's outputs as a caller of the step receives them (the graph and the node features, both in the
    graph's Morton order) -> ``outdir/<name>.npy``: features as float32, indices as float64 (exact).  Each of the four
    arrays gets a quarter of DUMP_BYTES; a larger one is cut to a fixed seeded sample of its rows, whose row indices are
    written beside it as ``<name>_rows.npy``."""
    os.makedirs(outdir, exist_ok=True)
    arrays = {"out": out.float(), "perm": g.perm, "rowptr": g.rowptr, "src": g.src}
    share = DUMP_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float32 if a.dtype.kind == "f" else np.float64)
        row_bytes = a.itemsize * (a.size // max(1, a.shape[0]))
        if a.nbytes > share:
            k = share // (row_bytes + 8)
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], size=k, replace=False))
            a = a[rows]
            np.save(os.path.join(outdir, f"{name}_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(outdir, f"{name}.npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", type=int, default=1_000_000, help="particles per GPU (weak scaling)")
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lmax", type=int, default=2, help="2 = the configuration BASELINE.json's metric is quoted on")
    ap.add_argument("--cpu-sample", type=int, default=None, help="particles in the CPU-baseline sample")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="storage type of features / weights (bf16 = BASELINE config 3; l_max=2 only)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: per-launch HIP events in the timed steps for "
                         "`roofline`, the bf16-storage leg and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0) as DIR/<name>.npy")
    ap.add_argument("--timing-json", type=str, default=None, help="also dump per-TP timings here (with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-bf16-leg", action="store_true",
                    help="with --full: skip the extra timed leg in bf16 storage (BASELINE.json configs[2]) reported as "
                         "`bf16_storage`")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.timing_json and not args.full:
        raise SystemExit("--timing-json needs --full (the per-launch timings come from its instrumented steps)")

    import models  # noqa: F401
    from scalable_e3_gnn_amd import ops, profiling
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    from scalable_e3_gnn_amd.segnn import SEGNN

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as plain `python bench.py --gpus N`: this process becomes the launcher of its N ranks.  It has not touched
        # the GPU (no HIP call so far), starts the ranks as child processes and exits with their worst return code.
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU path)")
    backend = os.environ.get("E3_BENCH_BACKEND", "nccl")  # "gloo": rehearsal of N ranks on fewer GPUs
    if backend == "gloo":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    if args.lmax not in (1, 2):
        raise SystemExit("l_max must be 1 or 2")
    if args.cpu_sample is None:
        args.cpu_sample = 20000 if args.lmax == 1 else 16000

    n = args.particles
    # One global cloud of world*n particles in [0,world) x [0,1)^2, cut into slabs along x: rank k owns
    # x in [k,k+1) (generated in place: synthetic data) and ghosts of width r from its slab neighbours.
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    pos = torch.rand(n, 3, device=dev, generator=gen)
    pos[:, 0] += float(rank)
    x = torch.randn(n, 4, device=dev, generator=gen)
    r = cutoff(n)
    torch.manual_seed(0)
    model = SEGNN("1x0e+1x1o", args.hidden, "1x1o", args.layers, lmax=args.lmax).to(dev)
    if args.dtype == "bf16":
        if args.lmax != 2:
            raise SystemExit("--dtype bf16 is implemented for --lmax 2")
        model = model.bfloat16()
        x = x.bfloat16()
    halo = None
    if world > 1:
        from scalable_e3_gnn_amd.sharding import SlabHalo
        halo = SlabHalo()
    lo = [float(rank) - (2 * r if world > 1 else 0.0), 0.0, 0.0]
    hi = [float(rank) + 1.0 + (2 * r if world > 1 else 0.0), 1.0, 1.0]

    def make_step(model, x):
        def step():
            split = None
            if halo is None:
                g = radius_graph(pos, r, lo, hi)
                xs = x[g.perm.long()]
            else:
                lpos, lx = halo.setup(pos, x, float(rank), float(rank + 1), r)   # ghost positions + features
                g = radius_graph(lpos, r, lo, hi)
                halo.renumber(g.perm)
                xs = lx[g.perm.long()]
                split = halo.split_graph(g)   # ghost-dst edges dropped; interior edges overlap the per-layer refresh
            with torch.no_grad():
                out = model(xs, g, halo=halo, split=split)
            return g, out
        return step

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, warmup, steps, profile):
        for _ in range(warmup):
            step()
        fence()
        if profile:
            profiling.enable()
        t0 = time.perf_counter()
        for _ in range(steps):
            g, out = step()
        fence()
        dt = time.perf_counter() - t0
        prof = profiling.summary() if profile else None
        if profile:
            profiling.disable()
        if dist is not None:
            t = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        assert torch.isfinite(out.float()).all()
        return dt, g, out, prof

    dt, g, out, prof = timed(make_step(model, x), args.warmup, args.steps, args.full)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, g, out)
    # second leg, same workload in bf16 storage (BASELINE.json configs[2]); reported beside the fp32 value, never as it
    bf16_leg = None
    if args.full and args.dtype == "f32" and args.lmax == 2 and not args.no_bf16_leg:
        m16 = SEGNN("1x0e+1x1o", args.hidden, "1x1o", args.layers, lmax=args.lmax).to(dev)
        m16.load_state_dict(model.state_dict())
        m16 = m16.bfloat16()
        dt16, _, _, prof16 = timed(make_step(m16, x.bfloat16()), max(1, args.warmup), args.steps, True)
        bf16_leg = {"value": n * world / (dt16 / args.steps), "unit": "particles/s", "ms_per_step": dt16 / args.steps * 1e3,
                    "dtype": "bf16", "steps": args.steps,
                    "numerics": "bf16 storage of features/weights/messages, fp32 spherical harmonics, bf16 MFMA with "
                                "fp32 accumulation; END TO END: the 4-layer H=32 l_max=2 model is within 6.8e-3 of the fp64 "
                                "oracle evaluated on the bf16-rounded model (tests/test_parity_bench_mode_gpu.py asserts <= 2e-2); "
                                "at this bench's size the fused message launch is within 8.0e-4 of the exact fp32 chain on "
                                "bf16-rounded operands at 500 sampled nodes (tests/test_fullsize_gpu.py asserts < 3e-3)"}
        if rank == 0 and prof16:
            tag16, dom16 = max(prof16.items(), key=lambda kv: kv[1]["total_ms"])
            bf16_leg["roofline"] = roofline_of(tag16, dom16, os.path.join(REPO, "profiles", f"r03_traffic_bf16_lmax{args.lmax}.json"))
        del m16
    if rank == 0:
        ms = dt / args.steps * 1e3
        total_particles = n * world
        roof = None
        if args.full:
            dom_tag, dom = max(prof.items(), key=lambda kv: kv[1]["total_ms"])
            roof = roofline_of(dom_tag, dom, os.path.join(REPO, "profiles", f"r03_traffic_lmax{args.lmax}.json"))
            roof["tp_share_of_step"] = sum(v["total_ms"] for v in prof.values()) / (dt * 1e3)
            if args.timing_json:
                json.dump(prof, open(args.timing_json, "w"), indent=1)
        line = {
            "metric": METRIC, "value": total_particles / (dt / args.steps), "unit": "particles/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "numerics": ("fp32 storage and accumulation; tensor-product contractions as fp16 (hi, lo)-split MFMA with "
                         "power-of-two operand scales (3 f16 MFMA products per fp32 product, fp32 accumulate): a 4-layer "
                         "H=32 forward is within 2.7e-7 (l_max=2) / 3.1e-7 (l_max=1) of the fp64 oracle in THIS mode -- "
                         "tests/test_parity_bench_mode_gpu.py asserts <= 1e-5 (north_star); the exact-fp32 FMA kernels give "
                         "2.0e-7, the torch-CPU fp32 port 1.8e-7")
                        if args.dtype == "f32" else
                        ("bf16 storage of features/weights/messages, fp32 spherical harmonics, bf16 MFMA with fp32 "
                         "accumulation (one TP within 1e-2 of the fp64 oracle on bf16-rounded inputs)"),
            "config": {"workload": f"{n} particles/GPU uniform in unit box, radius graph k~24 (E={g.num_edges}), "
                                   f"SEGNN l_max={args.lmax} {args.layers} layers H={args.hidden} {args.dtype} storage",
                       "particles_per_gpu": n, "edges_per_gpu": g.num_edges, "hidden": args.hidden,
                       "layers": args.layers, "lmax": args.lmax,
                       "parallelism": (f"spatial slabs x{world}, ghost halo width r, 1 position + {args.layers} feature "
                                       f"p2p exchanges/step over RCCL") if world > 1 else "single GPU"},
        }
        if roof is not None:
            line["roofline"] = roof
        if bf16_leg is not None:
            line["bf16_storage"] = bf16_leg
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], line["cpu_baseline_best_effort"] = cpu_baseline(args, model.state_dict())
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
