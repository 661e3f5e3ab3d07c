"""What the envelope costs in the aggregation.  e3_segment_sum_weighted and its backward against e3_segment_sum and its
backward on the same [E, D] operands in one process: E = 2.4 M edges in 100 k rows (k = 24 per row), D = 288 (hidden 32,
l_max = 2) by default -- 2.76 GB per [E, D] tensor, far past the Infinity Cache.

The legs alternate after a warm-up; every repeat is timed with device events and the medians are printed as one JSON line
with the bytes each leg has to move and the rate that gives.  Kernel times: run under `rocprofv3 --kernel-trace --stats`
(separately from this timing; `--repeats 3 --inner 1` keeps the trace short).

    python tools/envelope_micro.py [--rows N] [--degree K] [--width D] [--repeats R] [--inner I] [--warmup W]
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
from scalable_e3_gnn_amd import _lib  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--degree", type=int, default=24)
    ap.add_argument("--width", type=int, default=288)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, D = args.rows, args.width
    gen = torch.Generator(device=dev).manual_seed(0)
    # degrees k/2 .. 3k/2 (mean k): rows of a radius graph differ in length
    deg = torch.randint(args.degree // 2, args.degree + args.degree // 2 + 1, (N,), device=dev, generator=gen)
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0).int()
    E = int(rowptr[-1])
    msg = torch.randn(E, D, device=dev, generator=gen)
    w = torch.rand(E, device=dev, generator=gen)
    agg = torch.empty(N, D, device=dev)
    gagg = torch.randn(N, D, device=dev, generator=gen)
    gmsg = torch.empty(E, D, device=dev)
    gw = torch.empty(E, device=dev)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: t.data_ptr()

    legs = {
        "segment_sum": lambda: _lib.check(lib.e3_segment_sum(ptr(msg), D, ptr(rowptr), N, D, ptr(agg), D, st)),
        "segment_sum_weighted": lambda: _lib.check(lib.e3_segment_sum_weighted(ptr(msg), D, ptr(w), ptr(rowptr), N, D,
                                                                               ptr(agg), D, st)),
        "segment_sum_backward": lambda: _lib.check(lib.e3_segment_sum_backward(ptr(gagg), D, ptr(rowptr), N, D, ptr(gmsg), D,
                                                                               st)),
        "segment_sum_weighted_backward_gmsg": lambda: _lib.check(lib.e3_segment_sum_weighted_backward(
            ptr(gagg), D, None, D, ptr(w), ptr(rowptr), N, D, ptr(gmsg), D, None, st)),
        "segment_sum_weighted_backward": lambda: _lib.check(lib.e3_segment_sum_weighted_backward(
            ptr(gagg), D, ptr(msg), D, ptr(w), ptr(rowptr), N, D, ptr(gmsg), D, ptr(gw), st)),
    }
    # the weighted forward at w = 1 is the plain sum, bit for bit (checked once, outside the timing)
    legs["segment_sum"]()
    ref = agg.clone()
    _lib.check(lib.e3_segment_sum_weighted(ptr(msg), D, ptr(torch.ones_like(w)), ptr(rowptr), N, D, ptr(agg), D, st))
    assert torch.equal(ref, agg), "weighted sum at w = 1 differs from e3_segment_sum"
    row, node = 4 * E * D, 4 * N * D
    need = {"segment_sum": row + node, "segment_sum_weighted": row + node + 4 * E, "segment_sum_backward": row + node,
            "segment_sum_weighted_backward_gmsg": row + node + 4 * E, "segment_sum_weighted_backward": 2 * row + node + 8 * E}
    med, every = timed(legs, args.repeats, args.inner, args.warmup)
    print(json.dumps({"rows": N, "edges": E, "width": D, "median_ms": med, "repeats_ms": every,
                      "bytes_needed": need, "TB_per_s": {k: round(need[k] / med[k] * 1e-9, 3) for k in med}}))


if __name__ == "__main__":
    main()
