#!/usr/bin/env python3
"""L1TP operator micro-benchmark (rows/s, algorithmic GB/s) — development tool, not the judged bench."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import models  # noqa
from models.segnn.l1_tensor_prod import L1TensorProduct
from scalable_e3_gnn_amd import Irreps

ap = argparse.ArgumentParser()
ap.add_argument("--H", type=int, nargs="+", default=[32])
ap.add_argument("--B", type=int, default=1 << 21)
ap.add_argument("--kernels", type=int, nargs="*", default=[1, 2])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--irreps", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--dtype", choices=["fp32", "fp64", "bf16"], default="fp32")
ap.add_argument("--own-backward", action="store_true",
                help="route every backward to e3_l1tp_backward (the rows and weights kernels), whatever B, and time it alone")
ap.add_argument("--skip-backward", action="store_true", help="no forward + backward through autograd")
ap.add_argument("--lib", type=str, default=None, help="time this build of libe3gnn_hip.so (e.g. one kept from the parent)")
ap.add_argument("--json", type=str, default=None, help="append one JSON line per timing to this file")
a = ap.parse_args()
dev = "cuda:0"
dt = {"fp32": torch.float32, "fp64": torch.float64, "bf16": torch.bfloat16}[a.dtype]
if a.lib:
    from scalable_e3_gnn_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
if a.own_backward:
    from scalable_e3_gnn_amd import tensor_product
    tensor_product._BWD_GEMM_MIN_ROWS = 1 << 62


def record(what, ms):
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps({"what": what, "dtype": a.dtype, "B": a.B, "lib": a.lib or "tree", "ms": ms}) + "\n")


for H in a.H:
    ir = a.irreps or f"{H}x0e+{H}x1o"
    torch.manual_seed(0)
    mod = L1TensorProduct(Irreps(ir), Irreps(a.out) if a.out else None).to(dt).to(dev)
    x = torch.randn(a.B, mod.in1_dim, device=dev).to(dt)
    y = torch.randn(a.B, 4, device=dev).to(dt)
    Dout = mod.iro.dim
    ref = None
    for k in a.kernels:
        mod.kernel = k
        with torch.no_grad():
            try:
                o = mod(x, y)
            except RuntimeError as e:
                print(f"{ir} kernel={k}: {e}")
                continue
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                o = mod(x, y)
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        gb = x.element_size() * (mod.in1_dim + 4 + Dout) * a.B / 1e9
        record(f"forward kernel={k}", ms)
        err = 0.0 if ref is None else ((o - ref).abs().max() / ref.abs().max()).item()  # of the timed kernels
        if ref is None:
            ref = o.clone()
        print(f"{ir} -> {a.out or ir}  B={a.B} {a.dtype} kernel={k}: {ms:.3f} ms  {a.B / ms / 1e6:.1f} Grows/s*1e-3  "
              f"{gb / ms * 1e3:.0f} GB/s algorithmic  diff-vs-first {err:.1e}", flush=True)
    go = torch.randn(a.B, Dout, device=dev).to(dt)

    def timed(f, n):
        f(); f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    if a.own_backward:
        # e3_l1tp_backward alone: the rows kernel (grad_in1) and the two weight-gradient kernels
        ms = timed(lambda: mod._hip_backward(x, y, go, True, False, True), a.iters)
        record("e3_l1tp_backward (grad_in1, grad_W)", ms)
        print(f"{ir} -> {a.out or ir}  B={a.B} {a.dtype} e3_l1tp_backward (grad_in1, grad_W): {ms:.4f} ms", flush=True)
    if a.skip_backward:
        continue
    # forward + backward (grad_in1 and grad_W; in2 = harmonics of fixed positions needs none): the training use of the operator
    mod.kernel = 0
    xg = x.clone().requires_grad_(True)

    def fb():
        for p in mod.parameters():
            p.grad = None
        xg.grad = None
        mod(xg, y).backward(go)

    ms = timed(fb, max(1, a.iters // 2))
    record("forward + backward", ms)
    print(f"{ir} -> {a.out or ir}  B={a.B} {a.dtype} forward + backward (grad_in1, grad_W): {ms:.3f} ms  "
          f"{a.B / ms / 1e6:.2f} Grows/s*1e-3", flush=True)
