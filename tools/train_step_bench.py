#!/usr/bin/env python3
"""Forward + backward timings (development / profiles tool).

  (a) BASELINE.json configs[3]: 128 synthetic QM9-shaped molecules (3..29 atoms, positions randn * 1.5 A, r = 5 A), l_max = 2,
      4 layers, H = 32: energies + forces (-dE/dpos) + dE/dparam = one training step on energies with forces predicted;
  (b) BASELINE.json configs[1]: 100 k particles, l_max = 1, 4 layers, H = 32: forward + backward of sum(out^2) w.r.t. every
      parameter.
The one-launch fused kernels are inference kernels; a call that needs a gradient runs the differentiable chain (SEGNNLayer
warns once and names the reason): per-product forward kernels (MFMA where the shape has one) with [E, width] tensors
materialised, and the operands -> library GEMMs -> contract backward of tensor_product.tp_backward.  HIP-event times, ms per step after a warm-up.

usage: train_step_bench.py [--force-loss] [OUT.json]      (OUT.json: every case that ran, by name)
  --force-loss: instead of (a) and (b), case (a)'s model on a force-matching loss L = mean((F - F*)^2) + mean((E - E*)^2) with
      ``create_graph=True`` (second derivatives: every product of the backward is differentiated once more, about three
      forwards and three backwards each) beside its energy-only step, alternating, REPEATS times each: medians and all values
      (profiles/force_loss_train_step.json).
"""
import json, math, os, statistics, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import models  # noqa
from scalable_e3_gnn_amd.batched import BatchedEnergyModel
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

dev = "cuda:0"
iters = int(os.environ.get("ITERS", 5))
repeats = int(os.environ.get("REPEATS", 5))


def timed(fn):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def molecules():
    """case (a)'s batch and model -> (model, params, x, pos, batch, atoms)"""
    g = torch.Generator().manual_seed(3)
    counts = torch.randint(3, 30, (128,), generator=g)
    batch = torch.repeat_interleave(torch.arange(128), counts)
    N = int(counts.sum())
    pos = (torch.randn(N, 3, generator=g) * 1.5).to(dev)
    x = torch.randn(N, 4, generator=g).to(dev)
    torch.manual_seed(0)
    model = BatchedEnergyModel("1x0e+1x1o", 32, 4, lmax=2).to(dev).train()
    return model, [p for p in model.parameters() if p.requires_grad], x, pos, batch.to(dev), N


def energy_step(model, params, x, pos, batch):
    def step():
        for p in params:
            p.grad = None
        e, f = model(x, pos, batch, 5.0, forces=True)
        e.sum().backward()
    return step


def case_molecules():
    """(a) 128 molecules, l_max = 2, energy + force head"""
    model, params, x, pos, batch, N = molecules()

    def fwd():
        with torch.no_grad():
            return model(x, pos, batch, 5.0)

    model.eval(); t_inf = timed(fwd); model.train()
    t_train = timed(energy_step(model, params, x, pos, batch))
    return {"atoms": N, "forward_inference_ms": t_inf, "energy_forces_param_grads_ms": t_train,
            "note": "inference = fused MFMA kernels; training step = differentiable chain, backward = operands -> GEMMs -> "
                    "contract (forward with autograd graph, -dE/dpos, dE/dparam)"}


def case_force_loss():
    """case (a)'s model: a step on a force-matching loss beside the energy-only step of the same run"""
    model, params, x, pos, batch, N = molecules()
    with torch.no_grad():
        e_ref, f_ref = model(x, pos, batch, 5.0, forces=True)
    gt = torch.Generator().manual_seed(4)
    e_star = (e_ref + 0.1 * e_ref.abs().mean() * torch.randn(e_ref.shape, generator=gt).to(dev)).detach()
    f_star = (f_ref + 0.1 * f_ref.abs().mean() * torch.randn(f_ref.shape, generator=gt).to(dev)).detach()

    def force_step():
        for p in params:
            p.grad = None
        e, f = model(x, pos, batch, 5.0, forces=True, create_graph=True)
        ((f - f_star).square().mean() + (e - e_star).square().mean()).backward()

    step = energy_step(model, params, x, pos, batch)
    t_energy, t_force = [], []
    for _ in range(repeats):   # alternating, so that a drift of the clocks reaches both alike
        t_energy.append(timed(step))
        t_force.append(timed(force_step))
    me, mf = statistics.median(t_energy), statistics.median(t_force)
    return {"atoms": N, "energy_only_step_ms": me, "force_loss_step_ms": mf, "ratio": mf / me,
            "energy_only_step_ms_all": t_energy, "force_loss_step_ms_all": t_force, "steps_per_value": iters,
            "note": "same run, same model (128 molecules, l_max = 2, 4 layers, H = 32), medians of alternating measurements; "
                    "energy-only step = forward with graph, -dE/dpos, dE/dparam of sum E; force-loss step = the same forward, "
                    "-dE/dpos with create_graph=True, and dL/dparam of L = mean((F - F*)^2) + mean((E - E*)^2) through the "
                    "backward of the backward"}


def case_particles():
    """(b) 100 k particles, l_max = 1"""
    n = 100_000
    pos = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    xb = torch.randn(n, 4, device=dev)
    r = float((3.0 * 24.0 / (4.0 * math.pi * n)) ** (1.0 / 3.0))
    torch.manual_seed(0)
    m1 = SEGNN("1x0e+1x1o", 32, "1x1o", 4, lmax=1).to(dev)
    p1 = [p for p in m1.parameters() if p.requires_grad]
    gr = radius_graph(pos, r, [0, 0, 0], [1, 1, 1])
    xs = xb[gr.perm.long()]

    def step():
        for p in p1:
            p.grad = None
        o = m1(xs, gr)
        o.square().sum().backward()

    def fwd():
        with torch.no_grad():
            return m1(xs, gr)

    t_inf = timed(fwd)
    t_train = timed(step)
    return {"particles": n, "edges": gr.num_edges, "forward_inference_ms": t_inf, "forward_backward_ms": t_train,
            "note": "graph build excluded; inference = fused MFMA kernels; forward + backward = differentiable "
                    "chain ([E, width] tensors materialised), backward = operands -> GEMMs -> contract"}


def main(argv):
    files = [a for a in argv if not a.startswith("--")]
    cases = ({"qm9_128mol_lmax2_force_loss": case_force_loss} if "--force-loss" in argv else
             {"qm9_128mol_lmax2": case_molecules, "particles_100k_lmax1": case_particles})
    warnings.simplefilter("always")
    out = {}
    for name, case in cases.items():
        out[name] = case()
        print(json.dumps(out[name]), flush=True)
    if files:
        with open(files[0], "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
